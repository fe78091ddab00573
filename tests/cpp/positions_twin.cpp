// Host twin of the tree-pose and global-positioning calls of local-features_amd/csrc/mkd_positions.hip: the kernels' own
// arithmetic (csrc/mkd_positions_math.h, compiled here by a plain C++ compiler with -ffp-contract=off) under a serial
// restatement of what the kernels do with it -- gp_tree_poses' walk up the chain and its sum from the root down, gp_init,
// gp_gauge's sums with camera i in slot i mod 256 and position p in slot p mod 256 through rs_combine, gp_points' sums with
// position lo + j in slot j mod 4 through tri_combine, gp_cameras' sums with row lo + j in slot j mod 256, and the two final
// kernels.  Counts are integer sums and the minimum of the cosines has one answer in any order, so the serial order is the
// device's.  No arithmetic of its own beyond the sine of the robust angle, formed as lf_mkd_global_positions_device forms it.
// tests/positions_twin.py drives it:
//
//   positions_twin IN OUT      IN = calls back to back, OUT = their results back to back
//
//   a tree call: u32 0, n_images, n_edges, max_depth, fill; u32 edge_a[n_edges], edge_b[n_edges]; f32 t[n_edges][3],
//       rotations[n_images][9]; u32 image_stats[n_images][4]
//   ->  u32 poses[n_images][12]
//   a positions call: u32 1, n_images, sweeps, warm, min_obs, fill, with_points, with_state, with_trace, 0; f32 robust_deg, 0;
//       u64 n_rows, track_capacity, obs_capacity; u32 table_counts[2]; u64 image_offsets[n_images + 1],
//       track_offsets[track_capacity + 1]; f32 kps[n_rows][5]; i32 row_track[n_rows], obs_row[obs_capacity]; u32
//       obs_image[obs_capacity]; f32 intrinsics[n_images][4], poses[n_images][12]
//   ->  u32 poses_out[n_images][12], points[track_capacity][4] (with_points), obs_state[obs_capacity] (with_state),
//       image_stats[n_images][4]; f64 trace[sweeps][4] (with_trace); u32 counts[8] -- every word `fill` where the call writes
//       nothing
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mkd_positions_math.h"

using namespace lfmkd;

namespace {

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "positions_twin: input ends early\n");
        exit(2);
    }
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "positions_twin: cannot write\n");
        exit(2);
    }
}
unsigned word(float v) {
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}
uint64_t clamp_to(uint64_t v, uint64_t total) { return v < total ? v : total; }

// ---- tree poses ---------------------------------------------------------------------------------------------------------------
struct Tree {
    unsigned n_images, n_edges, max_depth, fill;
    std::vector<unsigned> edge_a, edge_b, stats;
    std::vector<float> t, rot;
};
bool tree_up(const Tree &c, unsigned j, unsigned &parent, double *step) {
    const unsigned e = c.stats[4 * size_t(j) + 2];
    if (e >= c.n_edges) return false;
    const unsigned a = c.edge_a[e], b = c.edge_b[e];
    if (a >= c.n_images || b >= c.n_images || a == b || (j != a && j != b)) return false;
    double u[3];
    if (!gp_tree_step(&c.rot[9 * size_t(b)], &c.t[3 * size_t(e)], u)) return false;
    parent = j == a ? b : a;
    for (int k = 0; k < 3; ++k) step[k] = j == b ? u[k] : 0.0 - u[k];
    return true;
}
void run_tree(FILE *in, FILE *out) {
    Tree c;
    unsigned head[4];
    get(in, head, 4);
    c.n_images = head[0], c.n_edges = head[1], c.max_depth = head[2], c.fill = head[3];
    const size_t n = c.n_images, E = c.n_edges;
    c.edge_a.resize(E), c.edge_b.resize(E), c.t.resize(3 * E), c.rot.resize(9 * n), c.stats.resize(4 * n);
    get(in, c.edge_a.data(), E), get(in, c.edge_b.data(), E), get(in, c.t.data(), 3 * E), get(in, c.rot.data(), 9 * n);
    get(in, c.stats.data(), 4 * n);
    std::vector<unsigned> poses(12 * n, c.fill);
    for (unsigned i = 0; i < c.n_images; ++i) {
        unsigned depth = 0, j = i;
        bool ok = true;
        double step[3];
        while (true) {
            if (c.stats[4 * size_t(j) + 1] == kGpNone || !gp_rotation_set(&c.rot[9 * size_t(j)])) ok = false;
            if (!ok || c.stats[4 * size_t(j) + 1] == 0u) break;
            unsigned parent = j;
            if (depth == c.max_depth || !tree_up(c, j, parent, step)) ok = false;
            if (!ok) break;
            j = parent;
            ++depth;
        }
        float row[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ok) {
            // the chain's images, i first; the steps are added from the root's child down
            std::vector<unsigned> chain(1, i);
            for (unsigned k = 0; k < depth; ++k) {
                unsigned parent;
                tree_up(c, chain.back(), parent, step);
                chain.push_back(parent);
            }
            double cen[3] = {0.0, 0.0, 0.0};
            for (unsigned m = depth; m >= 1; --m) {
                unsigned parent;
                tree_up(c, chain[m - 1], parent, step);
                for (int k = 0; k < 3; ++k) cen[k] = cen[k] + step[k];
            }
            for (int k = 0; k < 9; ++k) row[k] = c.rot[9 * size_t(i) + k];
            gp_translation(row, cen, row + 9);
        }
        for (int k = 0; k < 12; ++k) poses[12 * size_t(i) + k] = word(row[k]);
    }
    put(out, poses.data(), poses.size());
}

// ---- global positions ---------------------------------------------------------------------------------------------------------
struct Call {
    unsigned n_images, sweeps, warm, min_obs, fill, with_points, with_state, with_trace;
    float robust_deg;
    uint64_t n_rows, tcap, ocap;
    unsigned tc[2];
    std::vector<uint64_t> ioff, toff;
    std::vector<float> kps, K, poses;
    std::vector<int> row_track, obs_row;
    std::vector<unsigned> obs_image;
    // the scratch
    std::vector<double> cen, pt;
    std::vector<float> rot;
    std::vector<unsigned> reg, held, reason, tflag;
    unsigned w_held = 0, w_unsolved = 0;
    uint64_t T, O;
};
struct Rule {
    double s0;
    unsigned min_obs;
    bool robust;
};
void image_range(const Call &c, unsigned img, uint64_t &lo, uint64_t &hi) {
    lo = clamp_to(c.ioff[img], c.n_rows);
    hi = clamp_to(c.ioff[img + 1], c.n_rows);
    hi = hi > lo ? hi : lo;
}
void track_range(const Call &c, uint64_t t, uint64_t &lo, uint64_t &hi) {
    lo = clamp_to(c.toff[t], c.O);
    hi = clamp_to(c.toff[t + 1], c.O);
    hi = hi > lo ? hi : lo;
}
bool obs_ray(const Call &c, uint64_t pos, unsigned &img, double *v) {
    const int row = c.obs_row[pos];
    img = c.obs_image[pos];
    if (row < 0 || uint64_t(row) >= c.n_rows || img >= c.n_images || !c.reg[img]) return false;
    const float x = c.kps[5 * size_t(row)], y = c.kps[5 * size_t(row) + 1];
    if (!tri_keypoint_usable(x, y)) return false;
    gp_ray(x, y, &c.K[4 * size_t(img)], &c.rot[9 * size_t(img)], v);
    return true;
}
bool row_ray(const Call &c, uint64_t r, unsigned img, uint64_t &t, double *v) {
    const int tr = c.row_track[r];
    if (tr < 0 || uint64_t(tr) >= c.T) return false;
    const float x = c.kps[5 * r], y = c.kps[5 * r + 1];
    if (!tri_keypoint_usable(x, y)) return false;
    t = uint64_t(tr);
    gp_ray(x, y, &c.K[4 * size_t(img)], &c.rot[9 * size_t(img)], v);
    return true;
}

void gauge(Call &c, const Rule &rule, unsigned sweep, std::vector<double> &trace, std::vector<unsigned> &counts) {
    static double slot[3][kRsSlots];
    const auto zero = [&]() {
        for (int k = 0; k < 3; ++k)
            for (int s = 0; s < kRsSlots; ++s) slot[k][s] = 0.0;
    };
    zero();
    unsigned n_reg = 0;
    for (unsigned i = 0; i < c.n_images; ++i) {
        if (!c.reg[i]) continue;
        for (int k = 0; k < 3; ++k) slot[k][i % kRsSlots] = slot[k][i % kRsSlots] + c.cen[3 * size_t(i) + k];
        ++n_reg;
    }
    double m[3];
    for (int k = 0; k < 3; ++k) m[k] = rs_combine(slot[k]) / double(n_reg);
    zero();
    for (unsigned i = 0; i < c.n_images; ++i) {
        if (!c.reg[i]) continue;
        const double *p = &c.cen[3 * size_t(i)];
        const double d[3] = {p[0] - m[0], p[1] - m[1], p[2] - m[2]};
        slot[0][i % kRsSlots] = slot[0][i % kRsSlots] + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    const double rho = sqrt(rs_combine(slot[0]) / double(n_reg));
    const bool ok = n_reg > 0 && gp_finite3(m) && pose_finite(rho) && rho > 0.0;
    if (ok) {
        for (unsigned i = 0; i < c.n_images; ++i)
            if (c.reg[i]) gp_regauge(&c.cen[3 * size_t(i)], m, rho);
        for (uint64_t t = 0; t < c.T; ++t) gp_regauge(&c.pt[3 * t], m, rho);
    }
    if (!ok) counts[kGpCGaugeFailed] += 1u;
    if (sweep == kGpNone) return;
    if (c.with_trace) {
        zero();
        unsigned weighted = 0;
        for (uint64_t p = 0; p < c.O; ++p) {
            unsigned img;
            double v[3];
            if (!obs_ray(c, p, img, v)) continue;
            const int t = c.row_track[c.obs_row[p]];
            if (t < 0 || uint64_t(t) >= c.T || !(c.tflag[t] & 1u)) continue;
            const double *X = &c.pt[3 * size_t(t)], *cn = &c.cen[3 * size_t(img)];
            const double w = gp_weight(v, X, cn, rule.s0, rule.robust);
            if (!(w > 0.0)) continue;
            double pr2, rr, depth;
            gp_residual(v, X, cn, pr2, rr, depth);
            slot[0][p % kRsSlots] = slot[0][p % kRsSlots] + w * pr2;
            ++weighted;
        }
        double *row = &trace[4 * size_t(sweep)];
        row[0] = rs_combine(slot[0]), row[1] = double(weighted), row[2] = double(c.w_held), row[3] = double(c.w_unsolved);
    }
    counts[kGpCHeld] = c.w_held;
    c.w_held = c.w_unsolved = 0;
}

void points_step(Call &c, const Rule &rule) {
    for (uint64_t t = 0; t < c.T; ++t) {
        uint64_t lo, hi;
        track_range(c, t, lo, hi);
        const bool before = (c.tflag[t] & 1u) != 0;
        double X0[3] = {c.pt[3 * t], c.pt[3 * t + 1], c.pt[3 * t + 2]};
        double slot[kGpTerms][kTriSlots];
        for (int k = 0; k < kGpTerms; ++k)
            for (int s = 0; s < kTriSlots; ++s) slot[k][s] = 0.0;
        unsigned weighted = 0;
        for (uint64_t pos = lo; pos < hi; ++pos) {
            unsigned img;
            double v[3], term[kGpTerms];
            if (!obs_ray(c, pos, img, v)) continue;
            const double *cn = &c.cen[3 * size_t(img)];
            const double w = gp_weight(v, X0, cn, rule.s0, rule.robust && before);
            if (!(w > 0.0)) continue;
            gp_terms(v, w, cn, term);
            const int s = int((pos - lo) % kTriSlots);
            for (int k = 0; k < kGpTerms; ++k) slot[k][s] = slot[k][s] + term[k];
            ++weighted;
        }
        double sums[kGpTerms], X[3];
        for (int k = 0; k < kGpTerms; ++k) sums[k] = tri_combine(slot[k]);
        const bool solved = gp_solve(sums, weighted, rule.min_obs, X) == kGpSolved;
        if (solved)
            for (int k = 0; k < 3; ++k) c.pt[3 * t + k] = X[k];
        c.tflag[t] = solved ? 1u : 0u;
        if (!solved) ++c.w_unsolved;
    }
}

void cameras_step(Call &c, const Rule &rule) {
    static double slot[kGpTerms][kRsSlots];
    for (unsigned img = 0; img < c.n_images; ++img) {
        if (!c.reg[img]) continue;
        uint64_t lo, hi;
        image_range(c, img, lo, hi);
        const double cn[3] = {c.cen[3 * size_t(img)], c.cen[3 * size_t(img) + 1], c.cen[3 * size_t(img) + 2]};
        for (int k = 0; k < kGpTerms; ++k)
            for (int s = 0; s < kRsSlots; ++s) slot[k][s] = 0.0;
        unsigned weighted = 0;
        for (uint64_t r = lo; r < hi; ++r) {
            uint64_t t;
            double v[3], term[kGpTerms];
            if (!row_ray(c, r, img, t, v) || !(c.tflag[t] & 1u)) continue;
            const double *X = &c.pt[3 * t];
            const double w = gp_weight(v, X, cn, rule.s0, rule.robust);
            if (!(w > 0.0)) continue;
            gp_terms(v, w, X, term);
            const int s = int((r - lo) % kRsSlots);
            for (int k = 0; k < kGpTerms; ++k) slot[k][s] = slot[k][s] + term[k];
            ++weighted;
        }
        double sums[kGpTerms], out[3];
        for (int k = 0; k < kGpTerms; ++k) sums[k] = rs_combine(slot[k]);
        const unsigned reason = gp_solve(sums, weighted, rule.min_obs, out);
        c.reason[img] = reason;
        if (reason == kGpSolved)
            for (int k = 0; k < 3; ++k) c.cen[3 * size_t(img) + k] = out[k];
        else {
            c.held[img] += 1u;
            ++c.w_held;
        }
    }
}

void run_positions(FILE *in, FILE *out) {
    Call c;
    unsigned head[9];
    float fl[2];
    uint64_t sizes[3];
    get(in, head, 9), get(in, fl, 2), get(in, sizes, 3), get(in, c.tc, 2);
    c.n_images = head[0], c.sweeps = head[1], c.warm = head[2], c.min_obs = head[3], c.fill = head[4];
    c.with_points = head[5], c.with_state = head[6], c.with_trace = head[7];
    c.robust_deg = fl[0];
    c.n_rows = sizes[0], c.tcap = sizes[1], c.ocap = sizes[2];
    const size_t n = c.n_images;
    c.ioff.resize(n + 1), c.toff.resize(c.tcap + 1), c.kps.resize(5 * c.n_rows), c.row_track.resize(c.n_rows);
    c.obs_row.resize(c.ocap), c.obs_image.resize(c.ocap), c.K.resize(4 * n), c.poses.resize(12 * n);
    get(in, c.ioff.data(), n + 1), get(in, c.toff.data(), c.tcap + 1), get(in, c.kps.data(), 5 * c.n_rows);
    get(in, c.row_track.data(), c.n_rows), get(in, c.obs_row.data(), c.ocap), get(in, c.obs_image.data(), c.ocap);
    get(in, c.K.data(), 4 * n), get(in, c.poses.data(), 12 * n);
    c.T = clamp_to(c.tc[0], c.tcap), c.O = clamp_to(c.tc[1], c.ocap);

    std::vector<unsigned> poses_out(12 * n, c.fill), points(c.with_points ? 4 * c.tcap : 0, c.fill);
    std::vector<unsigned> state(c.with_state ? c.ocap : 0, c.fill), image_stats(4 * n, c.fill), counts(8, c.fill);
    std::vector<double> trace(c.with_trace ? 4 * size_t(c.sweeps) : 0);
    for (size_t i = 0; i < trace.size(); ++i) {
        const uint64_t both = uint64_t(c.fill) << 32 | c.fill;
        memcpy(&trace[i], &both, 8);
    }
    if (n) {
        const double s0 = sin(double(c.robust_deg) * (3.14159265358979323846 / 180.0));
        const auto rule_of = [&](unsigned sweep) { return Rule{s0, c.min_obs, sweep >= c.warm}; };
        // gp_init
        c.cen.assign(3 * n, 0.0), c.pt.assign(3 * c.tcap, 0.0), c.rot.assign(9 * n, 0.f);
        c.reg.assign(n, 0u), c.held.assign(n, 0u), c.reason.assign(n, 0u), c.tflag.assign(c.tcap, 0u);
        for (size_t i = 0; i < n; ++i) {
            const float *K = &c.K[4 * i], *P = &c.poses[12 * i];
            const bool reg = tri_camera_usable(K, P);
            if (reg) gp_centre(K, P, &c.cen[3 * i]);
            for (int k = 0; k < 9; ++k) c.rot[9 * i + k] = reg ? P[k] : 0.f;
            c.reg[i] = reg ? 1u : 0u;
            c.reason[i] = reg ? kGpSolved : kGpNotRegistered;
        }
        for (int k = 0; k < 8; ++k) counts[k] = k == kGpCSweeps ? c.sweeps : 0u;
        gauge(c, rule_of(0), kGpNone, trace, counts);
        for (unsigned s = 0; s < c.sweeps; ++s) {
            points_step(c, rule_of(s));
            cameras_step(c, rule_of(s));
            gauge(c, rule_of(s), s, trace, counts);
        }
        const Rule last = c.sweeps ? rule_of(c.sweeps - 1) : Rule{s0, c.min_obs, false};
        // gp_final_images
        for (unsigned img = 0; img < c.n_images; ++img) {
            unsigned *row = &poses_out[12 * size_t(img)], *st = &image_stats[4 * size_t(img)];
            if (!c.reg[img]) {
                for (int k = 0; k < 12; ++k) row[k] = word(0.f);
                st[0] = st[1] = st[2] = 0u, st[3] = kGpNotRegistered;
                continue;
            }
            uint64_t lo, hi;
            image_range(c, img, lo, hi);
            const double *cn = &c.cen[3 * size_t(img)];
            unsigned usable = 0, weighted = 0;
            for (uint64_t r = lo; r < hi; ++r) {
                uint64_t t;
                double v[3];
                if (!row_ray(c, r, img, t, v) || !(c.tflag[t] & 1u)) continue;
                ++usable;
                weighted += gp_state(true, true, gp_weight(v, &c.pt[3 * t], cn, last.s0, last.robust)) == 2u ? 1u : 0u;
            }
            float tr[3];
            gp_translation(&c.rot[9 * size_t(img)], cn, tr);
            for (int k = 0; k < 9; ++k) row[k] = word(c.rot[9 * size_t(img) + k]);
            for (int k = 0; k < 3; ++k) row[9 + k] = word(tr[k]);
            st[0] = usable, st[1] = weighted, st[2] = c.held[img], st[3] = c.reason[img];
            counts[kGpCRegistered] += 1u, counts[kGpCUsable] += usable, counts[kGpCWeighted] += weighted;
        }
        // gp_final_tracks
        counts[kGpCTracks] = unsigned(c.T);
        for (uint64_t t = 0; t < c.T; ++t) {
            uint64_t lo, hi;
            track_range(c, t, lo, hi);
            const bool solved = (c.tflag[t] & 1u) != 0;
            const double *X = &c.pt[3 * t];
            uint64_t first = ~0ull;
            double va[3] = {0.0, 0.0, 0.0}, cosine = 2.0;
            for (uint64_t pos = lo; pos < hi; ++pos) {
                unsigned img;
                double v[3], w = 0.0;
                const bool usable = obs_ray(c, pos, img, v);
                if (usable && solved) w = gp_weight(v, X, &c.cen[3 * size_t(img)], last.s0, last.robust);
                if (c.with_state) state[pos] = gp_state(usable, solved, w);
                if (!(w > 0.0)) continue;
                if (first == ~0ull) {
                    first = pos;
                    for (int k = 0; k < 3; ++k) va[k] = v[k];
                } else {
                    const double cs = tri_cosine(va, v);
                    cosine = cs < cosine ? cs : cosine;
                }
            }
            if (c.with_points) {
                unsigned *p = &points[4 * t];
                p[0] = word(solved ? float(X[0]) : 0.f), p[1] = word(solved ? float(X[1]) : 0.f);
                p[2] = word(solved ? float(X[2]) : 0.f), p[3] = word(solved ? float(cosine) : 2.f);
            }
            if (solved) counts[kGpCSolvedPoints] += 1u;
        }
    }
    put(out, poses_out.data(), poses_out.size()), put(out, points.data(), points.size()), put(out, state.data(), state.size());
    put(out, image_stats.data(), image_stats.size()), put(out, trace.data(), trace.size()), put(out, counts.data(), counts.size());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: positions_twin IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "positions_twin: cannot open the files\n");
        return 2;
    }
    unsigned kind;
    while (fread(&kind, 4, 1, in) == 1) {
        if (kind == 0) run_tree(in, out);
        else run_positions(in, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
