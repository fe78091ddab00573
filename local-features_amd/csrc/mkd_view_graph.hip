// gfx950 view-graph checks (include/lf_mkd.h, lf_mkd_view_graph_device): the triangle vote over the posed edges of
// an edge list, the global rotations of the images by a breadth-first tree and lazy quaternion averaging over the kept edges,
// per-edge residuals and the match array with the dropped edges' entries at -1.  The arithmetic is csrc/mkd_view_graph_math.h,
// which the host twin compiles too.
//
// The pairs live in a table T uint32 [n_images][n_images] in the handle's scratch: T[i][j] = T[j][i] = the lowest usable edge
// index of the pair {i, j} (its representative), 0xFFFFFFFF for none.  The launches, in order:
//   vg_zero     T = none, the image statistics' start values, the counts = 0 (a kernel, not a memset node)
//   vg_edges    a thread per edge: usable?, its quaternion (f64, into the scratch), an integer atomic min into T (both ways)
//   vg_vote     a wave per edge (a, b): rows T[a][.] and T[b][.] walked together 64 columns at a time; a lane whose column c has
//               both pairs forms the loop's quaternion; closed and consistent are popcounts of ballots.  Lane 0 writes the
//               edge's statistics and adds to its two images' counters (integer atomics: no order in them)
//   vg_root     one workgroup: the given root, or the largest (kept edges, lowest id) over the images
//   vg_tree     x tree_rounds, a wave per image without a rotation: its row, the best kept edge to an image labelled in an
//               earlier round by a 64-bit key and a wave-wide maximum.  A round reads the labels it writes only as "not
//               labelled before this round" (either value of a label being written answers the same), and a quaternion only
//               of an image labelled in an earlier launch
//   vg_sweep    x iterations, a wave per labelled image, from one quaternion array into the other: its row in ascending j, the
//               hit lanes' predictions compacted into LDS in that order, sixteen lanes (slot, component) add the terms of
//               their slot in ascending order, lane 0 combines
//   vg_final    a thread per image and per edge: the rotations, the residuals and the five edge counts (a popcount per wave
//               and one integer add per wave and count: an add per edge in vg_vote was measured at 1.06 ms for 32 262 edges, the
//               adds queueing on five words; profiles/view_graph.md)
//   vg_filter   only with a match array: a workgroup per edge, its range of entries copied or set to -1
// No floating-point atomic, no workgroup waits for another, nothing is read back, no allocation.  (n_edges == 0: no vg_edges,
// vg_vote and vg_filter.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_view_graph_math.h"

namespace lfmkd {
namespace {

constexpr int kThreads = 256, kWave = 64;

__device__ __forceinline__ VgQuat load_quat(const double *q, uint64_t i) {
    return VgQuat{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
}
__device__ __forceinline__ void store_quat(double *q, uint64_t i, const VgQuat &v) {
    q[4 * i] = v.w, q[4 * i + 1] = v.x, q[4 * i + 2] = v.y, q[4 * i + 3] = v.z;
}
// the quaternion x -> (the other end) of representative `rep`: stored as (edge_a, edge_b), conjugated if x is not edge_a
__device__ __forceinline__ VgQuat from_image(const double *qe, const unsigned *edge_a, unsigned rep, unsigned x) {
    return vg_directed(load_quat(qe, rep), edge_a[rep] != x);
}

__global__ __launch_bounds__(kThreads) void vg_zero(unsigned *__restrict__ table, uint64_t cells, unsigned n_images,
                                                    unsigned *__restrict__ image_stats, unsigned *__restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < cells) table[i] = kVgNone;
    if (i < n_images) {
        image_stats[4 * i] = 0u;
        image_stats[4 * i + 1] = kVgNone;
        image_stats[4 * i + 2] = kVgNone;
        image_stats[4 * i + 3] = 0u;
    }
    if (i < 8) counts[i] = 0u;
}

__global__ __launch_bounds__(kThreads) void vg_edges(const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                     unsigned n_edges, const float *__restrict__ R,
                                                     const unsigned *__restrict__ pose_stats, unsigned n_images, unsigned min_front,
                                                     unsigned *__restrict__ table, double *__restrict__ qe,
                                                     unsigned *__restrict__ edge_stats) {
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_edges) return;
    const unsigned a = edge_a[e], b = edge_b[e];
    float Rf[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rf[i] = R[9 * e + i];
    const bool usable = vg_usable(a, b, n_images, pose_stats + 4 * e, Rf, min_front);
    // (element 3 marks the usable edges for vg_vote, which writes the four words of those)
    edge_stats[4 * e] = 0u, edge_stats[4 * e + 1] = 0u, edge_stats[4 * e + 2] = kVgUnusable;
    edge_stats[4 * e + 3] = usable ? (unsigned)e : kVgNone;
    if (!usable) return;
    store_quat(qe, e, vg_from_rotation(Rf));
    atomicMin(table + (uint64_t)a * n_images + b, (unsigned)e);
    atomicMin(table + (uint64_t)b * n_images + a, (unsigned)e);
}

__global__ __launch_bounds__(kWave) void vg_vote(const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                 unsigned n_images, const unsigned *__restrict__ table,
                                                 const double *__restrict__ qe, double cmax, bool use_unchecked,
                                                 unsigned *__restrict__ edge_stats, unsigned *__restrict__ image_stats) {
    const unsigned e = blockIdx.x, lane = threadIdx.x;
    if (edge_stats[4 * (uint64_t)e + 3] == kVgNone) return;                       // workgroup-uniform
    const unsigned a = edge_a[e], b = edge_b[e];
    const unsigned *row_a = table + (uint64_t)a * n_images, *row_b = table + (uint64_t)b * n_images;
    const VgQuat q_e = load_quat(qe, e);
    unsigned closed = 0, consistent = 0;
    for (unsigned c0 = 0; c0 < n_images; c0 += kWave) {                           // wave-uniform: the ballots see whole waves
        const unsigned c = c0 + lane;
        bool hit = false, ok = false;
        if (c < n_images && c != a && c != b) {
            const unsigned ra = row_a[c], rb = row_b[c];
            hit = ra != kVgNone && rb != kVgNone;
            if (hit) ok = vg_loop_closes(from_image(qe, edge_a, ra, c), from_image(qe, edge_a, rb, b), q_e, cmax);
        }
        closed += (unsigned)__popcll(__ballot(hit));
        consistent += (unsigned)__popcll(__ballot(ok));
    }
    if (lane != 0) return;
    const unsigned rep = row_a[b], state = vg_state(closed, consistent);
    unsigned *st = edge_stats + 4 * (uint64_t)e;
    st[0] = closed, st[1] = consistent, st[2] = state, st[3] = rep;
    // (the five edge counts are vg_final's: one add per edge here on a handful of words is what the launch would wait for)
    if (rep == e && vg_kept_state(state, use_unchecked)) {
        atomicAdd(image_stats + 4 * (uint64_t)a, 1u);
        atomicAdd(image_stats + 4 * (uint64_t)b, 1u);
    }
    if (state == kVgRejected) {
        atomicAdd(image_stats + 4 * (uint64_t)a + 3, 1u);
        atomicAdd(image_stats + 4 * (uint64_t)b + 3, 1u);
    }
}

// labelled: does the call count its root (not when there is no edge: every count is then 0)
__global__ __launch_bounds__(kThreads) void vg_root(unsigned n_images, unsigned root, bool have_edges, double *__restrict__ q,
                                                    unsigned *__restrict__ image_stats, unsigned *__restrict__ counts) {
    __shared__ unsigned long long s_best[kThreads];
    const unsigned tid = threadIdx.x;
    if (root == kVgNone) {
        if (!have_edges) return;                                                  // no edge: no image is labelled
        unsigned long long best = 0;
        for (unsigned i = tid; i < n_images; i += kThreads) {
            const unsigned long long key = ((unsigned long long)image_stats[4 * (uint64_t)i] << 32) | (0xFFFFFFFFu - i);
            best = key > best ? key : best;
        }
        s_best[tid] = best;
        __syncthreads();
        for (unsigned m = kThreads / 2; m >= 1; m >>= 1) {
            if (tid < m) s_best[tid] = s_best[tid] > s_best[tid + m] ? s_best[tid] : s_best[tid + m];
            __syncthreads();
        }
        root = 0xFFFFFFFFu - (unsigned)(s_best[0] & 0xFFFFFFFFu);
    }
    if (tid != 0) return;
    image_stats[4 * (uint64_t)root + 1] = 0u;
    store_quat(q, root, VgQuat{1.0, 0.0, 0.0, 0.0});
    if (have_edges) counts[5] = 1u, counts[6] = root;
}

__device__ __forceinline__ bool kept_edge(const unsigned *edge_stats, unsigned rep, bool use_unchecked) {
    return vg_kept_state(edge_stats[4 * (uint64_t)rep + 2], use_unchecked);
}

__global__ __launch_bounds__(kWave) void vg_tree(unsigned round, const unsigned *__restrict__ edge_a,
                                                 const unsigned *__restrict__ edge_b, unsigned n_images,
                                                 const unsigned *__restrict__ table, const double *__restrict__ qe,
                                                 const unsigned *__restrict__ pose_stats, const unsigned *__restrict__ edge_stats,
                                                 bool use_unchecked, double *q, unsigned *image_stats, unsigned *__restrict__ counts) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    if (image_stats[4 * (uint64_t)i + 1] != kVgNone) return;                      // workgroup-uniform
    const unsigned *row = table + (uint64_t)i * n_images;
    unsigned long long best = 0;
    for (unsigned j = lane; j < n_images; j += kWave) {
        const unsigned rep = row[j];
        if (rep == kVgNone) continue;
        const unsigned state = edge_stats[4 * (uint64_t)rep + 2];
        // (a label another wave writes in this round reads as none or as `round`: not an earlier round either way)
        if (!vg_kept_state(state, use_unchecked) || image_stats[4 * (uint64_t)j + 1] >= round) continue;
        const unsigned long long key = vg_tree_key(state, pose_stats[4 * (uint64_t)rep], rep);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
        const unsigned long long other = __shfl_xor(best, m, kWave);
        best = other > best ? other : best;
    }
    if (lane != 0 || best == 0) return;
    const unsigned rep = vg_tree_key_edge(best);
    const unsigned j = edge_a[rep] == i ? edge_b[rep] : edge_a[rep];
    store_quat(q, i, vg_normalise(vg_predict(from_image(qe, edge_a, rep, j), load_quat(q, j))));
    image_stats[4 * (uint64_t)i + 1] = round;
    image_stats[4 * (uint64_t)i + 2] = rep;
    atomicAdd(counts + 5, 1u);
}

__global__ __launch_bounds__(kWave) void vg_sweep(const unsigned *__restrict__ edge_a, unsigned n_images,
                                                  const unsigned *__restrict__ table, const double *__restrict__ qe,
                                                  const unsigned *__restrict__ edge_stats, bool use_unchecked,
                                                  const unsigned *__restrict__ image_stats, const double *__restrict__ src,
                                                  double *__restrict__ dst) {
    __shared__ double s_p[kWave][4];
    __shared__ double s_slot[kVgSlots][4];
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    const unsigned label = image_stats[4 * (uint64_t)i + 1];
    if (label == kVgNone) return;                                                 // workgroup-uniform
    const VgQuat q_i = load_quat(src, i);
    if (label == 0u) {                                                            // the root keeps the identity
        if (lane == 0) store_quat(dst, i, q_i);
        return;
    }
    const unsigned *row = table + (uint64_t)i * n_images;
    const unsigned slot = lane >> 2, comp = lane & 3u;                            // lanes 0 .. 15: a slot's component
    double acc = 0.0;
    unsigned n = 0;
    for (unsigned j0 = 0; j0 < n_images; j0 += kWave) {                           // wave-uniform
        const unsigned j = j0 + lane;
        bool hit = false;
        unsigned rep = kVgNone;
        if (j < n_images) {
            rep = row[j];
            hit = rep != kVgNone && kept_edge(edge_stats, rep, use_unchecked) && image_stats[4 * (uint64_t)j + 1] != kVgNone;
        }
        const unsigned long long hits = __ballot(hit);
        const unsigned cnt = (unsigned)__popcll(hits);
        if (cnt == 0) continue;                                                   // wave-uniform
        if (hit) {
            const VgQuat p = vg_towards(vg_predict(from_image(qe, edge_a, rep, j), load_quat(src, j)), q_i);
            const unsigned at = (unsigned)__popcll(hits & ((1ull << lane) - 1ull));
            s_p[at][0] = p.w, s_p[at][1] = p.x, s_p[at][2] = p.y, s_p[at][3] = p.z;
        }
        __syncthreads();
        if (lane < 4 * kVgSlots)
            for (unsigned k = 0; k < cnt; ++k)
                if (((n + k) & (unsigned)(kVgSlots - 1)) == slot) acc = acc + s_p[k][comp];
        __syncthreads();
        n += cnt;
    }
    if (lane < 4 * kVgSlots) s_slot[slot][comp] = acc;
    __syncthreads();
    if (lane != 0) return;
    VgQuat sl[kVgSlots];
#pragma unroll
    for (int s = 0; s < kVgSlots; ++s) sl[s] = VgQuat{s_slot[s][0], s_slot[s][1], s_slot[s][2], s_slot[s][3]};
    store_quat(dst, i, vg_average(sl, n, q_i));
}

__global__ __launch_bounds__(kThreads) void vg_final(const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                     unsigned n_edges, unsigned n_images, const double *__restrict__ qe,
                                                     const double *__restrict__ q, const unsigned *__restrict__ edge_stats,
                                                     const unsigned *__restrict__ image_stats, bool use_unchecked,
                                                     float *__restrict__ rotations, float *__restrict__ residual,
                                                     unsigned *__restrict__ counts) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    // counts[0 .. 4]: usable, supported, rejected, unchecked, kept -- a popcount per wave, then one integer add per wave
    unsigned state = kVgUnusable;
    bool usable = false, kept = false;
    if (t < n_edges) {
        const unsigned *st = edge_stats + 4 * t;
        usable = st[3] != kVgNone;
        state = st[2];
        kept = usable && st[3] == (unsigned)t && vg_kept_state(state, use_unchecked);
    }
    const unsigned long long in[5] = {__ballot(usable), __ballot(state == kVgSupported), __ballot(state == kVgRejected),
                                      __ballot(state == kVgUnchecked), __ballot(kept)};
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (in[k]) atomicAdd(counts + k, (unsigned)__popcll(in[k]));
    }
    if (t < n_images) {
        float R[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (image_stats[4 * t + 1] != kVgNone) vg_rotation(load_quat(q, t), R);
#pragma unroll
        for (int k = 0; k < 9; ++k) rotations[9 * t + k] = R[k];
    }
    if (residual && t < n_edges) {
        float r = 2.f;
        if (edge_stats[4 * t + 3] != kVgNone) {
            const unsigned a = edge_a[t], b = edge_b[t];
            if (image_stats[4 * (uint64_t)a + 1] != kVgNone && image_stats[4 * (uint64_t)b + 1] != kVgNone)
                r = vg_residual(load_quat(q, b), load_quat(qe, t), load_quat(q, a));
        }
        residual[t] = r;
    }
}

__global__ __launch_bounds__(kThreads) void vg_filter(const uint64_t *__restrict__ edge_off, uint64_t capacity,
                                                      const unsigned *__restrict__ edge_stats, bool use_unchecked, const int *match,
                                                      int *match_out) {
    const unsigned e = blockIdx.x;
    const uint64_t lo_raw = edge_off[e], hi_raw = edge_off[e + 1];
    const uint64_t lo = lo_raw < capacity ? lo_raw : capacity, hi = hi_raw < capacity ? hi_raw : capacity;
    const unsigned *st = edge_stats + 4 * (uint64_t)e;
    const bool kept = st[3] == e && vg_kept_state(st[2], use_unchecked);
    for (uint64_t k = lo + threadIdx.x; k < hi; k += kThreads) match_out[k] = kept ? match[k] : -1;
}

unsigned blocks_of(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

ViewGraphPlan view_graph_plan(unsigned n_images, unsigned n_edges, unsigned tree_rounds, unsigned iterations, bool filter) {
    ViewGraphPlan p = {};
    if (n_images == 0) return p;
    p.launches = 3 + tree_rounds + iterations + (n_edges ? 2u + (filter ? 1u : 0u) : 0u);
    p.off_edge_quat = 0;
    p.off_quat[0] = p.off_edge_quat + 32 * (uint64_t)n_edges;
    p.off_quat[1] = p.off_quat[0] + 32 * (uint64_t)n_images;
    p.off_table = p.off_quat[1] + 32 * (uint64_t)n_images;
    p.scratch_bytes = p.off_table + 4 * (uint64_t)n_images * n_images;
    return p;
}

unsigned launch_view_graph(const ViewGraphPlan &plan, unsigned char *scratch, const unsigned *edge_a, const unsigned *edge_b,
                           unsigned n_edges, const float *R, const unsigned *pose_stats, unsigned n_images, double cmax,
                           unsigned min_front, unsigned root, unsigned tree_rounds, unsigned iterations, bool use_unchecked,
                           const uint64_t *edge_off, uint64_t capacity, const int *match, int *match_out, float *rotations,
                           unsigned *edge_stats, float *residual, unsigned *image_stats, unsigned *counts, hipStream_t stream) {
    if (n_images == 0) return 0;
    unsigned issued = 0;
    const auto launch = [&](auto kernel, unsigned grid, int threads, auto... args) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, stream, args...);
        ++issued;
    };
    double *qe = reinterpret_cast<double *>(scratch + plan.off_edge_quat);
    double *q[2] = {reinterpret_cast<double *>(scratch + plan.off_quat[0]), reinterpret_cast<double *>(scratch + plan.off_quat[1])};
    unsigned *table = reinterpret_cast<unsigned *>(scratch + plan.off_table);
    const uint64_t cells = (uint64_t)n_images * n_images;
    launch(vg_zero, blocks_of(cells > 8 ? cells : 8), kThreads, table, cells, n_images, image_stats, counts);
    if (n_edges) {
        launch(vg_edges, blocks_of(n_edges), kThreads, edge_a, edge_b, n_edges, R, pose_stats, n_images, min_front, table, qe, edge_stats);
        launch(vg_vote, n_edges, kWave, edge_a, edge_b, n_images, (const unsigned *)table, (const double *)qe, cmax, use_unchecked,
               edge_stats, image_stats);
    }
    launch(vg_root, 1u, kThreads, n_images, root, n_edges != 0, q[0], image_stats, counts);
    for (unsigned r = 1; r <= tree_rounds; ++r)
        launch(vg_tree, n_images, kWave, r, edge_a, edge_b, n_images, (const unsigned *)table, (const double *)qe, pose_stats,
               (const unsigned *)edge_stats, use_unchecked, q[0], image_stats, counts);
    for (unsigned it = 0; it < iterations; ++it)
        launch(vg_sweep, n_images, kWave, edge_a, n_images, (const unsigned *)table, (const double *)qe, (const unsigned *)edge_stats,
               use_unchecked, (const unsigned *)image_stats, (const double *)q[it & 1u], q[(it & 1u) ^ 1u]);
    launch(vg_final, blocks_of(n_images > n_edges ? n_images : n_edges), kThreads, edge_a, edge_b, n_edges, n_images,
           (const double *)qe, (const double *)q[iterations & 1u], (const unsigned *)edge_stats, (const unsigned *)image_stats,
           use_unchecked, rotations, residual, counts);
    if (n_edges && match_out)
        launch(vg_filter, n_edges, kThreads, edge_off, capacity, (const unsigned *)edge_stats, use_unchecked, match, match_out);
    return issued;
}

}  // namespace lfmkd
