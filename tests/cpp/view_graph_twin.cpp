// Host twin of the view-graph call of local-features_amd/csrc/mkd_view_graph.hip: the kernels' own arithmetic
// (csrc/mkd_view_graph_math.h, compiled here by a plain C++ compiler with -ffp-contract=off) under a serial restatement of what
// the kernels do with it -- vg_edges' usable test and the table of representatives (a minimum over edge indices), vg_vote's walk
// over the third image in ascending id with integer counts, vg_root's maximum over (kept edges, lowest id), vg_tree's
// level-synchronous rounds by the 64-bit key, vg_sweep's predictions in ascending neighbour id into slot (term mod 4) and the
// slots through vg_average, vg_final and vg_filter.  Counts are integer sums and the maxima are over total orders, so the serial
// order is the device's.  No arithmetic of its own beyond the cosine of the loop threshold, formed as lf_mkd_view_graph_device
// forms it.  tests/view_graph_twin.py drives it:
//
//   view_graph_twin IN OUT      IN = calls back to back, OUT = their results back to back
//
//   a call: u32 n_images, n_edges, min_front, root, tree_rounds, iterations, flags, fill, with_match (0 none, 1 into an array of
//       `fill`, 2 in place), with_residual; f32 max_loop_deg, 0; u64 n_entries; u32 edge_a[n_edges], edge_b[n_edges]; f32
//       R[n_edges][9]; u32 pose_stats[n_edges][4]; with_match != 0: u64 edge_offsets[n_edges + 1]; i32 match[n_entries]
//   ->  u32 rotations[n_images][9], edge_stats[n_edges][4], residual[n_edges], image_stats[n_images][4], counts[8],
//       match_out[n_entries] (with_match != 0) -- every word `fill` where the call writes nothing
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mkd_view_graph_math.h"

using namespace lfmkd;

namespace {

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "view_graph_twin: input ends early\n");
        exit(2);
    }
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "view_graph_twin: cannot write\n");
        exit(2);
    }
}

struct Call {
    unsigned n_images, n_edges, min_front, root, tree_rounds, iterations, flags, fill, with_match, with_residual;
    float deg;
    uint64_t n_entries;
    std::vector<unsigned> edge_a, edge_b, pose_stats;
    std::vector<float> R;
    std::vector<uint64_t> off;
    std::vector<int> match;
};

void run(const Call &c, FILE *out) {
    const size_t n = c.n_images, E = c.n_edges;
    const bool use_unchecked = (c.flags & 1u) != 0;
    const double cmax = cos(double(c.deg) * (3.14159265358979323846 / 180.0));
    std::vector<unsigned> rotations(9 * n, c.fill), edge_stats(4 * E, c.fill), residual(E, c.fill), image_stats(4 * n, c.fill);
    std::vector<unsigned> counts(8, c.fill), match_out(c.with_match ? c.n_entries : 0, c.fill);
    if (c.with_match == 2) memcpy(match_out.data(), c.match.data(), 4 * c.match.size());
    if (n) {
        std::vector<unsigned> table(n * n, kVgNone);
        std::vector<VgQuat> qe(E), q[2] = {std::vector<VgQuat>(n), std::vector<VgQuat>(n)};
        for (size_t i = 0; i < n; ++i) image_stats[4 * i] = image_stats[4 * i + 3] = 0u, image_stats[4 * i + 1] = image_stats[4 * i + 2] = kVgNone;
        for (int k = 0; k < 8; ++k) counts[k] = 0u;
        // vg_edges
        for (size_t e = 0; e < E; ++e) {
            const unsigned a = c.edge_a[e], b = c.edge_b[e];
            const bool usable = vg_usable(a, b, c.n_images, &c.pose_stats[4 * e], &c.R[9 * e], c.min_front);
            edge_stats[4 * e] = edge_stats[4 * e + 1] = 0u, edge_stats[4 * e + 2] = kVgUnusable, edge_stats[4 * e + 3] = usable ? unsigned(e) : kVgNone;
            if (!usable) continue;
            qe[e] = vg_from_rotation(&c.R[9 * e]);
            if (unsigned(e) < table[a * n + b]) table[a * n + b] = table[b * n + a] = unsigned(e);
        }
        const auto from_image = [&](unsigned rep, unsigned x) { return vg_directed(qe[rep], c.edge_a[rep] != x); };
        // vg_vote
        for (size_t e = 0; e < E; ++e) {
            if (edge_stats[4 * e + 3] == kVgNone) continue;
            const unsigned a = c.edge_a[e], b = c.edge_b[e];
            unsigned closed = 0, consistent = 0;
            for (unsigned t = 0; t < c.n_images; ++t) {
                if (t == a || t == b) continue;
                const unsigned ra = table[a * n + t], rb = table[b * n + t];
                if (ra == kVgNone || rb == kVgNone) continue;
                ++closed;
                consistent += vg_loop_closes(from_image(ra, t), from_image(rb, b), qe[e], cmax);
            }
            const unsigned rep = table[a * n + b], state = vg_state(closed, consistent);
            edge_stats[4 * e] = closed, edge_stats[4 * e + 1] = consistent, edge_stats[4 * e + 2] = state, edge_stats[4 * e + 3] = rep;
            ++counts[0];
            ++counts[state == kVgSupported ? 1 : state == kVgRejected ? 2 : 3];
            if (rep == e && vg_kept_state(state, use_unchecked)) ++counts[4], ++image_stats[4 * a], ++image_stats[4 * b];
            if (state == kVgRejected) ++image_stats[4 * a + 3], ++image_stats[4 * b + 3];
        }
        // vg_root
        unsigned root = c.root;
        if (root == kVgNone && E) {
            uint64_t best = 0;
            for (unsigned i = 0; i < c.n_images; ++i) {
                const uint64_t key = (uint64_t(image_stats[4 * i]) << 32) | (0xFFFFFFFFu - i);
                best = key > best ? key : best;
            }
            root = 0xFFFFFFFFu - unsigned(best & 0xFFFFFFFFu);
        }
        if (root != kVgNone) {
            image_stats[4 * root + 1] = 0u;
            q[0][root] = VgQuat{1.0, 0.0, 0.0, 0.0};
            if (E) counts[5] = 1u, counts[6] = root;
        }
        const auto kept = [&](unsigned rep) { return vg_kept_state(edge_stats[4 * rep + 2], use_unchecked); };
        // vg_tree
        for (unsigned r = 1; r <= c.tree_rounds; ++r)
            for (unsigned i = 0; i < c.n_images; ++i) {
                if (image_stats[4 * i + 1] != kVgNone) continue;
                uint64_t best = 0;
                for (unsigned j = 0; j < c.n_images; ++j) {
                    const unsigned rep = table[i * n + j];
                    if (rep == kVgNone || !kept(rep) || image_stats[4 * j + 1] >= r) continue;
                    const uint64_t key = vg_tree_key(edge_stats[4 * rep + 2], c.pose_stats[4 * rep], rep);
                    best = key > best ? key : best;
                }
                if (best == 0) continue;
                const unsigned rep = vg_tree_key_edge(best), j = c.edge_a[rep] == i ? c.edge_b[rep] : c.edge_a[rep];
                q[0][i] = vg_normalise(vg_predict(from_image(rep, j), q[0][j]));
                image_stats[4 * i + 1] = r, image_stats[4 * i + 2] = rep;
                ++counts[5];
            }
        // vg_sweep
        for (unsigned it = 0; it < c.iterations; ++it) {
            const std::vector<VgQuat> &src = q[it & 1u];
            std::vector<VgQuat> &dst = q[(it & 1u) ^ 1u];
            for (unsigned i = 0; i < c.n_images; ++i) {
                const unsigned label = image_stats[4 * i + 1];
                if (label == kVgNone) continue;
                if (label == 0u) {
                    dst[i] = src[i];
                    continue;
                }
                VgQuat slot[kVgSlots] = {};
                unsigned terms = 0;
                for (unsigned j = 0; j < c.n_images; ++j) {
                    const unsigned rep = table[i * n + j];
                    if (rep == kVgNone || !kept(rep) || image_stats[4 * j + 1] == kVgNone) continue;
                    const VgQuat p = vg_towards(vg_predict(from_image(rep, j), src[j]), src[i]);
                    VgQuat &s = slot[terms % kVgSlots];
                    s.w = s.w + p.w, s.x = s.x + p.x, s.y = s.y + p.y, s.z = s.z + p.z;
                    ++terms;
                }
                dst[i] = vg_average(slot, terms, src[i]);
            }
        }
        // vg_final
        const std::vector<VgQuat> &qf = q[c.iterations & 1u];
        for (unsigned i = 0; i < c.n_images; ++i) {
            float Rf[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (image_stats[4 * i + 1] != kVgNone) vg_rotation(qf[i], Rf);
            memcpy(&rotations[9 * size_t(i)], Rf, 36);
        }
        for (size_t e = 0; c.with_residual && e < E; ++e) {
            float r = 2.f;
            if (edge_stats[4 * e + 3] != kVgNone) {
                const unsigned a = c.edge_a[e], b = c.edge_b[e];
                if (image_stats[4 * a + 1] != kVgNone && image_stats[4 * b + 1] != kVgNone) r = vg_residual(qf[b], qe[e], qf[a]);
            }
            memcpy(&residual[e], &r, 4);
        }
        // vg_filter
        for (size_t e = 0; c.with_match && e < E; ++e) {
            const uint64_t lo = c.off[e] < c.n_entries ? c.off[e] : c.n_entries, hi = c.off[e + 1] < c.n_entries ? c.off[e + 1] : c.n_entries;
            const bool keep = edge_stats[4 * e + 3] == e && kept(unsigned(e));
            for (uint64_t k = lo; k < hi; ++k) match_out[k] = keep ? unsigned(c.match[k]) : 0xFFFFFFFFu;
        }
    }
    put(out, rotations.data(), rotations.size());
    put(out, edge_stats.data(), edge_stats.size());
    put(out, residual.data(), residual.size());
    put(out, image_stats.data(), image_stats.size());
    put(out, counts.data(), counts.size());
    put(out, match_out.data(), match_out.size());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: view_graph_twin IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "view_graph_twin: cannot open %s\n", in ? argv[2] : argv[1]);
        return 2;
    }
    unsigned h[10];
    while (fread(h, sizeof(unsigned), 10, in) == 10) {
        Call c;
        c.n_images = h[0], c.n_edges = h[1], c.min_front = h[2], c.root = h[3], c.tree_rounds = h[4], c.iterations = h[5], c.flags = h[6];
        c.fill = h[7], c.with_match = h[8], c.with_residual = h[9];
        float pad;
        get(in, &c.deg, 1);
        get(in, &pad, 1);
        get(in, &c.n_entries, 1);
        const size_t E = c.n_edges;
        c.edge_a.resize(E), c.edge_b.resize(E), c.R.resize(9 * E), c.pose_stats.resize(4 * E);
        get(in, c.edge_a.data(), E);
        get(in, c.edge_b.data(), E);
        get(in, c.R.data(), 9 * E);
        get(in, c.pose_stats.data(), 4 * E);
        if (c.with_match) {
            c.off.resize(E + 1);
            c.match.resize(c.n_entries);
            get(in, c.off.data(), E + 1);
            get(in, c.match.data(), c.match.size());
        }
        run(c, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
