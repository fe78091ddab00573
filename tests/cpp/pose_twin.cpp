// Host twin of the two-view pose call of local-features_amd/csrc/mkd_two_view_pose.hip: the kernel's own arithmetic
// (csrc/mkd_pose_math.h, compiled here by a plain C++ compiler with -ffp-contract=off) under a serial restatement of what the
// kernel's workgroup does with it -- the frame of an edge, the four counts over its links, the choice, the points and the
// parallax count.  Counts are integer sums, so the serial order is the workgroup's.  No arithmetic of its own beyond the
// cosine of the threshold, formed as lf_mkd_two_view_pose_device forms it.  tests/pose_twin.py drives it:
//
//   pose_twin IN OUT      IN = calls back to back, OUT = their results back to back
//
//   a call: u32 n_edges, n_images, fill; f32 min_parallax_deg; u64 n_rows, link_capacity; f32 kps[n_rows][5]; u32
//       edge_a[n_edges], edge_b[n_edges]; f32 intrinsics[n_images][4], F[n_edges][9]; u64 link_offsets[n_edges + 1]; i32
//       link_a[link_capacity], link_b[link_capacity]
//   ->  f32 R[n_edges][9], t[n_edges][3]; u32 stats[n_edges][4]; f32 sigma[n_edges][3]; u32 points[link_capacity][4] (every
//       word `fill` where the call writes nothing)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mkd_pose_math.h"

using namespace lfmkd;

namespace {

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "pose_twin: input ends early\n");
        exit(2);
    }
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "pose_twin: cannot write\n");
        exit(2);
    }
}

struct Call {
    unsigned n_edges, n_images, fill;
    float deg;
    uint64_t n_rows, cap;
    std::vector<float> kps, intr, F;
    std::vector<unsigned> ea, eb;
    std::vector<uint64_t> off;
    std::vector<int> la, lb;

    // load_link of the kernel
    bool link(uint64_t k, const float *Ka, const float *Kb, double *xa, double *xb) const {
        const int ra = la[k], rb = lb[k];
        if (ra < 0 || rb < 0 || uint64_t(ra) >= n_rows || uint64_t(rb) >= n_rows) return false;
        pose_ray(kps[5 * uint64_t(ra)], kps[5 * uint64_t(ra) + 1], Ka, xa);
        pose_ray(kps[5 * uint64_t(rb)], kps[5 * uint64_t(rb) + 1], Kb, xb);
        return true;
    }
};

void run(const Call &q, FILE *out) {
    const double cmin = cos(double(q.deg) * (3.14159265358979323846 / 180.0));
    std::vector<float> R(9 * size_t(q.n_edges)), t(3 * size_t(q.n_edges)), sigma(3 * size_t(q.n_edges));
    std::vector<unsigned> stats(4 * size_t(q.n_edges)), points(4 * q.cap, q.fill);
    for (unsigned e = 0; e < q.n_edges; ++e) {
        const uint64_t lo = q.off[e] < q.cap ? q.off[e] : q.cap, h0 = q.off[e + 1] < q.cap ? q.off[e + 1] : q.cap;
        const uint64_t hi = h0 > lo ? h0 : lo;
        const unsigned a = q.ea[e], b = q.eb[e];
        bool have = a < q.n_images && b < q.n_images;
        float K[8] = {};
        PoseFrame P = {};
        if (have) {
            for (int i = 0; i < 4; ++i) K[i] = q.intr[4 * size_t(a) + i], K[4 + i] = q.intr[4 * size_t(b) + i];
            double E[9];
            have = pose_essential(&q.F[9 * size_t(e)], K, K + 4, E);
            have = pose_decompose(E, P) && have;
        }
        unsigned cnt[4] = {0u, 0u, 0u, 0u};
        if (have)
            for (uint64_t k = lo; k < hi; ++k) {
                double xa[3], xb[3];
                if (!q.link(k, K, K + 4, xa, xb)) continue;
                const unsigned bits = pose_votes(P, xa, xb);
                for (int c = 0; c < 4; ++c) cnt[c] += (bits >> c) & 1u;
            }
        unsigned best = 0, other = 0;
        const unsigned c = have ? pose_choose(cnt, best, other) : kPoseNone;
        const bool pose = c != kPoseNone;
        double tt[3] = {0.0, 0.0, 0.0};
        const double *Rc = P.R[(c >> 1) & 1u];
        if (pose) pose_translation(P, c, tt);
        unsigned par = 0;
        for (uint64_t k = lo; k < hi; ++k) {
            double xa[3], xb[3];
            float o[4] = {0.f, 0.f, 0.f, 2.f};
            if (pose && q.link(k, K, K + 4, xa, xb)) {
                const PoseLink L = pose_link(Rc, tt, xa, xb);
                if (pose_front(L)) {
                    par += pose_parallax(L, cmin);
                    pose_point(Rc, tt, xa, xb, L, o);
                }
            }
            memcpy(&points[4 * k], o, 16);
        }
        for (int i = 0; i < 9; ++i) R[9 * size_t(e) + i] = pose ? float(Rc[i]) : 0.f;
        for (int i = 0; i < 3; ++i) {
            t[3 * size_t(e) + i] = pose ? float(tt[i]) : 0.f;
            sigma[3 * size_t(e) + i] = pose ? float(P.sigma[i]) : 0.f;
        }
        const unsigned st[4] = {pose ? best : 0u, pose ? other : 0u, c, par};
        memcpy(&stats[4 * size_t(e)], st, 16);
    }
    put(out, R.data(), R.size());
    put(out, t.data(), t.size());
    put(out, stats.data(), stats.size());
    put(out, sigma.data(), sigma.size());
    put(out, points.data(), points.size());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: pose_twin IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "pose_twin: cannot open %s\n", in ? argv[2] : argv[1]);
        return 2;
    }
    unsigned h[3];
    while (fread(h, sizeof(unsigned), 3, in) == 3) {
        Call q;
        q.n_edges = h[0], q.n_images = h[1], q.fill = h[2];
        get(in, &q.deg, 1);
        get(in, &q.n_rows, 1);
        get(in, &q.cap, 1);
        q.kps.resize(5 * q.n_rows);
        q.ea.resize(q.n_edges);
        q.eb.resize(q.n_edges);
        q.intr.resize(4 * size_t(q.n_images));
        q.F.resize(9 * size_t(q.n_edges));
        q.off.resize(size_t(q.n_edges) + 1);
        q.la.resize(q.cap);
        q.lb.resize(q.cap);
        get(in, q.kps.data(), q.kps.size());
        get(in, q.ea.data(), q.ea.size());
        get(in, q.eb.data(), q.eb.size());
        get(in, q.intr.data(), q.intr.size());
        get(in, q.F.data(), q.F.size());
        get(in, q.off.data(), q.off.size());
        get(in, q.la.data(), q.la.size());
        get(in, q.lb.data(), q.lb.size());
        run(q, out);
    }
    return fclose(out) == 0 ? 0 : 2;
}
