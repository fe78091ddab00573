// gfx950 tree poses and global positioning (include/lf_mkd.h, lf_mkd_tree_poses_device and lf_mkd_global_positions_device;
// DESIGN.md 6x): initial camera poses from the view graph's tree, then all camera centres and all track points at once under
// held rotations, by alternating weighted linear solves.  The arithmetic is csrc/mkd_positions_math.h, which the host twin
// compiles too.
//
//   gp_tree_poses    ONE launch, a thread per image: it walks its chain of tree edges up to the root to learn its depth, then
//                    adds the unit steps from the root down, so every word depends on the image's own chain alone.  The
//                    chain is taken 32 images at a time from the root's end: the thread walks up to the run (parents only:
//                    two loads a step), keeps the run's images in its own column of LDS and steps through them backwards --
//                    depth steps and depth^2 / 64 parent reads.
//
//   gp_init          a thread per image and per track: registered?, the centre, the rotation (kept in the scratch, so that
//                    the call may run in place), the counters and flags.
//   gp_gauge         ONE workgroup, before the first sweep and after every sweep: the mean and the rms radius of the
//                    registered centres in the 256-slot order (camera i in slot i mod 256), the similarity applied to the
//                    centres, and -- only with a trace -- the weighted cost over every observation (position p in slot p
//                    mod 256): THE COST PASS IS ONE WORKGROUP OVER ALL OBSERVATIONS.  The POINTS are not rewritten here: m
//                    and rho go to the scratch with a "pending" word, and whoever reads a point next -- gp_points of the next
//                    sweep, which stores every point again, the cost pass, the two final kernels -- applies (X - m) / rho on
//                    the read, the same operations on the same values.  (Rewriting all T points in this one workgroup was
//                    measured beside it: 51.7 against 186 us a sweep at 18 000 and 102 000 tracks; profiles/global_positions.md.)
//   gp_points        x sweeps.  4 lanes own a track (lane l reads positions lo + l, lo + 4 + l, ..: the lane is the slot of
//                    the 4-slot sum), the butterfly of track triangulation combines, tri_solve decides.
//   gp_cameras       x sweeps.  A workgroup owns an image and walks its rows 256 at a time (thread s is slot s of the
//                    256-slot sum); the workgroup sum is the butterfly within a wave, then ((w0 + w1) + w2) + w3.
//   gp_final_images  a workgroup per image: the pose, the image's statistics and its share of the counts.
//   gp_final_tracks  4 lanes per track: the final weights, the states, the point and its smallest cosine.
//
// 4 + 3 sweeps launches.  No floating-point atomic (the counters are integers: no order in them), no workgroup waits for
// another, nothing is read back, no allocation.  Every loop that holds a ballot or a lane permute runs in wave-uniform
// control flow.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_positions_math.h"
#include "mkd_scene.h"

namespace lfmkd {
namespace {

constexpr int kThreads = kRsSlots, kWaves = kThreads / 64, G = kTriSlots;
static_assert(kThreads == kSumThreads, "thread s is slot s of the canonical sum");
constexpr unsigned kMaxBlocks = 16384;                  // grid-stride beyond
// the scratch's words: cameras held and points unsolved in this sweep; is the latest gauge still to be applied to the points
enum : int { kWHeld = 0, kWUnsolved = 1, kWPending = 2 };
constexpr unsigned kPointSolved = 1u;
constexpr int kChainRun = 32;                           // images of a chain gp_tree_poses keeps at a time (32 KB of LDS)

// cen f64 [n_images][3], pt f64 [tcap][3], rot f32 [n_images][9], reg / held / reason uint32 [n_images], tflag uint32 [tcap],
// words uint32 [4], gauge f64 [4] = {m, rho} of the latest gauge
struct GpScratch {
    double *cen, *pt, *gauge;
    float *rot;
    unsigned *reg, *held, *reason, *tflag, *words;
};
// the weights' rule: robust or unit, the floor s0 of the sine, the fewest weighted observations of a solve
struct GpRule {
    double s0;
    unsigned min_obs;
    bool robust;
};

__device__ __forceinline__ void load3(const double *p, uint64_t i, double *v) { v[0] = p[3 * i], v[1] = p[3 * i + 1], v[2] = p[3 * i + 2]; }
__device__ __forceinline__ void store3(double *p, uint64_t i, const double *v) { p[3 * i] = v[0], p[3 * i + 1] = v[1], p[3 * i + 2] = v[2]; }
// The gauge that is still to be applied to the points (kernel-uniform), and point t under it.
struct Pending {
    double m[3], rho;
    bool on;
};
__device__ __forceinline__ Pending pending_gauge(const GpScratch &sc) {
    return Pending{{sc.gauge[0], sc.gauge[1], sc.gauge[2]}, sc.gauge[3], sc.words[kWPending] != 0u};
}
__device__ __forceinline__ void load_point(const GpScratch &sc, const Pending &g, uint64_t t, double *X) {
    load3(sc.pt, t, X);
    if (g.on) gp_regauge(X, g.m, g.rho);
}

// position `pos` of the observation arrays (pos < O): false if it is not usable; else its image and its world ray
__device__ __forceinline__ bool obs_ray(const SceneTables &in, const GpScratch &sc, uint64_t pos, unsigned &img, double *v) {
    const int row = in.obs_row[pos];
    img = in.obs_image[pos];
    if (row < 0 || (uint64_t)row >= in.n_rows || img >= in.n_images || !sc.reg[img]) return false;
    const float x = in.kps[5 * (uint64_t)row], y = in.kps[5 * (uint64_t)row + 1];
    if (!tri_keypoint_usable(x, y)) return false;
    float K[4], R[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = sc.rot[9 * (uint64_t)img + i];
    gp_ray(x, y, K, R, v);
    return true;
}
// row r of registered image img (lo <= r < hi <= n_rows): false if it is in no track below T or its keypoint is not finite;
// else its track and its world ray
__device__ __forceinline__ bool row_ray(const SceneTables &in, uint64_t r, uint64_t T, const float *K, const float *R, uint64_t &t, double *v) {
    const int tr = in.row_track[r];
    if (tr < 0 || (uint64_t)tr >= T) return false;
    const float x = in.kps[5 * r], y = in.kps[5 * r + 1];
    if (!tri_keypoint_usable(x, y)) return false;
    t = (uint64_t)tr;
    gp_ray(x, y, K, R, v);
    return true;
}

// ---- tree poses ---------------------------------------------------------------------------------------------------------------
struct TreeIn {
    const unsigned *__restrict__ edge_a, *__restrict__ edge_b;
    const float *__restrict__ t;
    unsigned n_edges;
    const float *__restrict__ rotations;
    const unsigned *__restrict__ stats;
    unsigned n_images;
};
// image j's step up its tree edge: false if the chain breaks here; else its parent and the signed unit step parent -> j
__device__ __forceinline__ bool tree_up(const TreeIn &in, unsigned j, unsigned &parent, double *step) {
    const unsigned e = in.stats[4 * (uint64_t)j + 2];
    if (e >= in.n_edges) return false;
    const unsigned a = in.edge_a[e], b = in.edge_b[e];
    if (a >= in.n_images || b >= in.n_images || a == b || (j != a && j != b)) return false;
    float Rb[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rb[i] = in.rotations[9 * (uint64_t)b + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = in.t[3 * (uint64_t)e + i];
    double u[3];
    if (!gp_tree_step(Rb, t, u)) return false;
    parent = j == a ? b : a;
#pragma unroll
    for (int k = 0; k < 3; ++k) step[k] = j == b ? u[k] : 0.0 - u[k];
    return true;
}
// image j's parent alone (its chain was walked by tree_up before: the indices are in range)
__device__ __forceinline__ unsigned tree_parent(const TreeIn &in, unsigned j) {
    const unsigned e = in.stats[4 * (uint64_t)j + 2], a = in.edge_a[e];
    return j == a ? in.edge_b[e] : a;
}
__device__ __forceinline__ bool tree_labelled(const TreeIn &in, unsigned j) {
    float R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = in.rotations[9 * (uint64_t)j + i];
    return in.stats[4 * (uint64_t)j + 1] != kGpNone && gp_rotation_set(R);
}

}  // namespace

__global__ __launch_bounds__(kThreads) void gp_tree_poses(TreeIn in, unsigned max_depth, float *__restrict__ poses) {
    __shared__ unsigned s_chain[kChainRun][kThreads];                             // [.][thread]: a thread's own column
    const unsigned tid = threadIdx.x;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= in.n_images) return;
    const unsigned i = (unsigned)gid;
    unsigned depth = 0, j = i;
    bool ok = true;
    double step[3];
    while (true) {
        if (!tree_labelled(in, j)) ok = false;
        if (!ok || in.stats[4 * (uint64_t)j + 1] == 0u) break;
        unsigned parent = j;
        if (depth == max_depth || !tree_up(in, j, parent, step)) ok = false;
        if (!ok) break;
        j = parent;
        ++depth;
    }
    float row[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) row[k] = 0.f;
    if (ok) {
        double c[3] = {0.0, 0.0, 0.0};
        // the chain's images are i = number 0, its parent = number 1, ..; the steps are those of numbers depth - 1 .. 0
        for (unsigned hi = depth; hi >= 1;) {
            const unsigned lo = hi > (unsigned)kChainRun ? hi - (unsigned)kChainRun : 0u;
            unsigned node = i;
            for (unsigned k = 0; k < lo; ++k) node = tree_parent(in, node);
            for (unsigned k = lo; k < hi; ++k) {
                s_chain[k - lo][tid] = node;
                node = tree_parent(in, node);
            }
            for (unsigned k = hi; k-- > lo;) {                                    // the root's end first
                unsigned parent;
                tree_up(in, s_chain[k - lo][tid], parent, step);
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = c[q] + step[q];
            }
            hi = lo;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) row[k] = in.rotations[9 * (uint64_t)i + k];
        gp_translation(row, c, row + 9);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) poses[12 * (uint64_t)i + k] = row[k];
}

// ---- global positions ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gp_init(SceneTables in, const float *__restrict__ poses, GpScratch sc, unsigned sweeps,
                                                    unsigned *__restrict__ counts) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, n = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = gid; i < in.n_images; i += n) {
        float K[4], P[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) K[k] = in.intrinsics[4 * i + k];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = poses[12 * i + k];
        const bool reg = tri_camera_usable(K, P);
        double c[3] = {0.0, 0.0, 0.0};
        if (reg) gp_centre(K, P, c);
        store3(sc.cen, i, c);
#pragma unroll
        for (int k = 0; k < 9; ++k) sc.rot[9 * i + k] = reg ? P[k] : 0.f;
        sc.reg[i] = reg ? 1u : 0u;
        sc.held[i] = 0u;
        sc.reason[i] = reg ? kGpSolved : kGpNotRegistered;
    }
    for (uint64_t t = gid; t < in.tcap; t += n) {
        const double zero[3] = {0.0, 0.0, 0.0};
        store3(sc.pt, t, zero);
        sc.tflag[t] = 0u;
    }
    if (gid < 4) sc.words[gid] = 0u;
    if (gid < 8) counts[gid] = gid == kGpCSweeps ? sweeps : 0u;
}

// sweep: kGpNone for the gauge before the first sweep (no trace row)
__global__ __launch_bounds__(kThreads) void gp_gauge(SceneTables in, GpScratch sc, GpRule rule, unsigned sweep, double *__restrict__ trace,
                                                     unsigned *__restrict__ counts) {
    __shared__ double s_red[kWaves * 3];
    __shared__ unsigned s_cnt;
    const unsigned tid = threadIdx.x;
    const uint64_t T = clamp_to(in.counts[0], in.tcap), O = clamp_to(in.counts[1], in.ocap);
    double acc[3] = {0.0, 0.0, 0.0};
    unsigned n_reg = 0;
    for (unsigned i = tid; i < in.n_images; i += kThreads) {
        if (!sc.reg[i]) continue;
        double c[3];
        load3(sc.cen, i, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + c[k];
        ++n_reg;
    }
    block_sum<double, 3>(acc, s_red);
    n_reg = block_count(n_reg, &s_cnt);
    const double m[3] = {acc[0] / double(n_reg), acc[1] / double(n_reg), acc[2] / double(n_reg)};
    double spread[1] = {0.0};
    for (unsigned i = tid; i < in.n_images; i += kThreads) {
        if (!sc.reg[i]) continue;
        double c[3];
        load3(sc.cen, i, c);
        const double d[3] = {c[0] - m[0], c[1] - m[1], c[2] - m[2]};
        spread[0] = spread[0] + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    block_sum<double, 1>(spread, s_red);
    const double rho = sqrt(spread[0] / double(n_reg));
    const bool ok = n_reg > 0 && gp_finite3(m) && pose_finite(rho) && rho > 0.0;   // block-uniform
    if (ok) {
        for (unsigned i = tid; i < in.n_images; i += kThreads) {
            if (!sc.reg[i]) continue;
            double c[3];
            load3(sc.cen, i, c);
            gp_regauge(c, m, rho);
            store3(sc.cen, i, c);
        }
    }
    const Pending now = {{m[0], m[1], m[2]}, rho, ok};
    __syncthreads();
    double cost[1] = {0.0};
    unsigned weighted = 0;
    if (trace && sweep != kGpNone) {                                              // block-uniform
        for (uint64_t p = tid; p < O; p += kThreads) {
            unsigned img;
            double v[3];
            if (!obs_ray(in, sc, p, img, v)) continue;
            const int t = in.row_track[in.obs_row[p]];
            if (t < 0 || (uint64_t)t >= T || !(sc.tflag[t] & kPointSolved)) continue;
            double X[3], c[3], pr2, rr, depth;
            load_point(sc, now, (uint64_t)t, X);
            load3(sc.cen, img, c);
            const double w = gp_weight(v, X, c, rule.s0, rule.robust);
            if (!(w > 0.0)) continue;
            gp_residual(v, X, c, pr2, rr, depth);
            cost[0] = cost[0] + w * pr2;
            ++weighted;
        }
        block_sum<double, 1>(cost, s_red);
        weighted = block_count(weighted, &s_cnt);
    }
    if (tid != 0) return;
    if (!ok) counts[kGpCGaugeFailed] += 1u;                                       // (one workgroup, stream-ordered: no atomic needed)
    sc.gauge[0] = m[0], sc.gauge[1] = m[1], sc.gauge[2] = m[2], sc.gauge[3] = rho;
    sc.words[kWPending] = ok ? 1u : 0u;
    if (sweep == kGpNone) return;
    if (trace) {
        double *row = trace + 4 * (uint64_t)sweep;
        row[0] = cost[0], row[1] = double(weighted), row[2] = double(sc.words[kWHeld]), row[3] = double(sc.words[kWUnsolved]);
    }
    counts[kGpCHeld] = sc.words[kWHeld];
    sc.words[kWHeld] = 0u, sc.words[kWUnsolved] = 0u;
}

__global__ __launch_bounds__(kThreads) void gp_points(SceneTables in, GpScratch sc, GpRule rule) {
    const TrackWalk w = track_walk(in);
    const Pending gauge = pending_gauge(sc);
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < w.T;
        uint64_t lo = 0, hi = 0;
        bool before = false;
        double X0[3] = {0.0, 0.0, 0.0};
        if (alive) {
            track_range(in, t, w.O, lo, hi);
            before = (sc.tflag[t] & kPointSolved) != 0;
            load_point(sc, gauge, t, X0);
        }
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);
        double acc[kGpTerms];
#pragma unroll
        for (int k = 0; k < kGpTerms; ++k) acc[k] = 0.0;
        unsigned weighted = 0;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            bool on = false;
            unsigned img;
            double v[3];
            if (ch < nch && pos < hi && obs_ray(in, sc, pos, img, v)) {
                double c[3], term[kGpTerms];
                load3(sc.cen, img, c);
                const double wt = gp_weight(v, X0, c, rule.s0, rule.robust && before);
                on = wt > 0.0;
                if (on) {
                    gp_terms(v, wt, c, term);
#pragma unroll
                    for (int k = 0; k < kGpTerms; ++k) acc[k] = acc[k] + term[k];
                }
            }
            weighted += (unsigned)__popc(group_bits(on, w.base));
        }
        double sums[kGpTerms], X[3];
#pragma unroll
        for (int k = 0; k < kGpTerms; ++k) sums[k] = combine(acc[k]);
        const bool solved = gp_solve(sums, weighted, rule.min_obs, X) == kGpSolved;
        const bool writer = alive && w.l == 0;
        if (writer) {
            store3(sc.pt, t, solved ? X : X0);                                    // (an unsolved point keeps its value, in the gauge)
            sc.tflag[t] = solved ? kPointSolved : 0u;
        }
        count_wave(writer && !solved, sc.words + kWUnsolved);
    }
}

__global__ __launch_bounds__(kThreads) void gp_cameras(SceneTables in, GpScratch sc, GpRule rule) {
    __shared__ double s_red[kWaves * kGpTerms];
    __shared__ unsigned s_cnt;
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    if (!sc.reg[img]) return;                                                     // block-uniform
    const uint64_t T = clamp_to(in.counts[0], in.tcap);
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    float K[4], R[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = sc.rot[9 * (uint64_t)img + i];
    double c[3];
    load3(sc.cen, img, c);
    double acc[kGpTerms];
#pragma unroll
    for (int k = 0; k < kGpTerms; ++k) acc[k] = 0.0;
    unsigned weighted = 0;
    for (uint64_t r = lo + tid; r < hi; r += kThreads) {
        uint64_t t;
        double v[3];
        if (!row_ray(in, r, T, K, R, t, v) || !(sc.tflag[t] & kPointSolved)) continue;
        double X[3], term[kGpTerms];
        load3(sc.pt, t, X);
        const double wt = gp_weight(v, X, c, rule.s0, rule.robust);
        if (!(wt > 0.0)) continue;
        gp_terms(v, wt, X, term);
#pragma unroll
        for (int k = 0; k < kGpTerms; ++k) acc[k] = acc[k] + term[k];
        ++weighted;
    }
    block_sum<double, kGpTerms>(acc, s_red);
    weighted = block_count(weighted, &s_cnt);
    double cn[3];
    const unsigned reason = gp_solve(acc, weighted, rule.min_obs, cn);
    if (tid != 0) return;
    sc.reason[img] = reason;
    if (reason == kGpSolved) store3(sc.cen, img, cn);
    else {
        sc.held[img] += 1u;
        atomicAdd(sc.words + kWHeld, 1u);
    }
}

__global__ __launch_bounds__(kThreads) void gp_final_images(SceneTables in, GpScratch sc, GpRule rule, float *__restrict__ poses_out,
                                                            unsigned *__restrict__ image_stats, unsigned *__restrict__ counts) {
    __shared__ unsigned s_cnt;
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    float *row = poses_out + 12 * (uint64_t)img;
    unsigned *st = image_stats + 4 * (uint64_t)img;
    if (!sc.reg[img]) {                                                           // block-uniform
        if (tid < 12) row[tid] = 0.f;
        if (tid < 4) st[tid] = tid == 3 ? kGpNotRegistered : 0u;
        return;
    }
    const uint64_t T = clamp_to(in.counts[0], in.tcap);
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    float K[4], R[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = sc.rot[9 * (uint64_t)img + i];
    double c[3];
    load3(sc.cen, img, c);
    unsigned usable = 0, weighted = 0;
    const Pending gauge = pending_gauge(sc);
    for (uint64_t r = lo + tid; r < hi; r += kThreads) {
        uint64_t t;
        double v[3];
        if (!row_ray(in, r, T, K, R, t, v) || !(sc.tflag[t] & kPointSolved)) continue;
        double X[3];
        load_point(sc, gauge, t, X);
        ++usable;
        weighted += gp_state(true, true, gp_weight(v, X, c, rule.s0, rule.robust)) == 2u ? 1u : 0u;
    }
    usable = block_count(usable, &s_cnt);
    weighted = block_count(weighted, &s_cnt);
    if (tid != 0) return;
    float t[3];
    gp_translation(R, c, t);
#pragma unroll
    for (int k = 0; k < 9; ++k) row[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) row[9 + k] = t[k];
    st[0] = usable, st[1] = weighted, st[2] = sc.held[img], st[3] = sc.reason[img];
    atomicAdd(counts + kGpCRegistered, 1u);
    if (usable) atomicAdd(counts + kGpCUsable, usable);
    if (weighted) atomicAdd(counts + kGpCWeighted, weighted);
}

__global__ __launch_bounds__(kThreads) void gp_final_tracks(SceneTables in, GpScratch sc, GpRule rule, float *__restrict__ points_out,
                                                            unsigned *__restrict__ obs_state, unsigned *__restrict__ counts) {
    const TrackWalk w = track_walk(in);
    const Pending gauge = pending_gauge(sc);
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[kGpCTracks] = (unsigned)w.T;
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < w.T;
        uint64_t lo = 0, hi = 0;
        bool solved = false;
        double X[3] = {0.0, 0.0, 0.0};
        if (alive) {
            track_range(in, t, w.O, lo, hi);
            solved = (sc.tflag[t] & kPointSolved) != 0;
            load_point(sc, gauge, t, X);
        }
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);
        // the first finally weighted position, and the states
        uint64_t first = ~0ull;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            const bool in_track = ch < nch && pos < hi;
            bool usable = false, on = false;
            double wt = 0.0;
            if (in_track) {
                unsigned img;
                double v[3], c[3];
                usable = obs_ray(in, sc, pos, img, v);
                if (usable && solved) {
                    load3(sc.cen, img, c);
                    wt = gp_weight(v, X, c, rule.s0, rule.robust);
                    on = wt > 0.0;
                }
                if (obs_state) obs_state[pos] = gp_state(usable, solved, wt);
            }
            const unsigned m = group_bits(on, w.base);
            if (m && first == ~0ull) first = lo + (uint64_t)ch * G + ((unsigned)__ffs((int)m) - 1u);
        }
        // the smallest cosine between its ray and each later weighted one
        double va[3] = {0.0, 0.0, 0.0}, cosine = 2.0;
        const bool have = solved && first != ~0ull;
        if (have) {
            unsigned img;
            obs_ray(in, sc, first, img, va);
        }
        for (unsigned ch = 0; __any(have && ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            if (have && ch < nch && pos < hi && pos > first) {
                unsigned img;
                double v[3], c[3];
                if (obs_ray(in, sc, pos, img, v)) {
                    load3(sc.cen, img, c);
                    if (gp_weight(v, X, c, rule.s0, rule.robust) > 0.0) {
                        const double cs = tri_cosine(va, v);
                        cosine = cs < cosine ? cs : cosine;
                    }
                }
            }
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
            const double other = __shfl_xor(cosine, m, 64);
            cosine = other < cosine ? other : cosine;
        }
        const bool writer = alive && w.l == 0;
        if (writer && points_out) {
            float *p = points_out + 4 * t;
            p[0] = solved ? float(X[0]) : 0.f;
            p[1] = solved ? float(X[1]) : 0.f;
            p[2] = solved ? float(X[2]) : 0.f;
            p[3] = solved ? float(cosine) : 2.f;
        }
        count_wave(writer && solved, counts + kGpCSolvedPoints);
    }
}

namespace {
unsigned blocks_of(uint64_t n) {
    const uint64_t want = (n + kThreads - 1) / kThreads;
    return (unsigned)(want < 1 ? 1 : want < kMaxBlocks ? want : kMaxBlocks);
}
uint64_t align16(uint64_t v) { return (v + 15) / 16 * 16; }
}  // namespace

void launch_tree_poses(const unsigned *edge_a, const unsigned *edge_b, const float *t, unsigned n_edges, const float *rotations,
                       const unsigned *image_stats, unsigned n_images, unsigned max_depth, float *poses, hipStream_t stream) {
    if (n_images == 0) return;
    const TreeIn in = {edge_a, edge_b, t, n_edges, rotations, image_stats, n_images};
    hipLaunchKernelGGL(gp_tree_poses, dim3((n_images + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, in, max_depth, poses);
}

GlobalPositionsPlan global_positions_plan(unsigned n_images, uint64_t track_capacity, unsigned sweeps) {
    GlobalPositionsPlan p = {};
    if (n_images == 0) return p;
    p.launches = 4 + 3 * sweeps;
    p.off_cen = 0;
    p.off_pt = align16(p.off_cen + 24 * (uint64_t)n_images);
    p.off_rot = align16(p.off_pt + 24 * track_capacity);
    p.off_reg = align16(p.off_rot + 36 * (uint64_t)n_images);
    p.off_held = align16(p.off_reg + 4 * (uint64_t)n_images);
    p.off_reason = align16(p.off_held + 4 * (uint64_t)n_images);
    p.off_tflag = align16(p.off_reason + 4 * (uint64_t)n_images);
    p.off_words = align16(p.off_tflag + 4 * track_capacity);
    p.off_gauge = p.off_words + 16;
    p.scratch_bytes = p.off_gauge + 32;
    return p;
}

unsigned launch_global_positions(const GlobalPositionsPlan &plan, unsigned char *scratch, const SceneTables &in, const float *poses,
                                 unsigned sweeps, unsigned warm, double s0, unsigned min_obs, float *poses_out, float *points_out,
                                 unsigned *obs_state, unsigned *image_stats, double *trace, unsigned *counts, hipStream_t stream) {
    const unsigned n_images = in.n_images;
    const uint64_t track_capacity = in.tcap;
    if (n_images == 0) return 0;
    unsigned issued = 0;
    const auto launch = [&](auto kernel, unsigned grid, auto... args) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, stream, args...);
        ++issued;
    };
    const GpScratch sc = {reinterpret_cast<double *>(scratch + plan.off_cen),     reinterpret_cast<double *>(scratch + plan.off_pt),
                          reinterpret_cast<double *>(scratch + plan.off_gauge),
                          reinterpret_cast<float *>(scratch + plan.off_rot),      reinterpret_cast<unsigned *>(scratch + plan.off_reg),
                          reinterpret_cast<unsigned *>(scratch + plan.off_held),  reinterpret_cast<unsigned *>(scratch + plan.off_reason),
                          reinterpret_cast<unsigned *>(scratch + plan.off_tflag), reinterpret_cast<unsigned *>(scratch + plan.off_words)};
    const unsigned track_blocks = blocks_of(track_capacity * G);
    const auto rule_of = [&](unsigned sweep) { return GpRule{s0, min_obs, sweep >= warm}; };
    launch(gp_init, blocks_of(n_images > track_capacity ? n_images : track_capacity), in, poses, sc, sweeps, counts);
    launch(gp_gauge, 1u, in, sc, rule_of(0), kGpNone, trace, counts);
    for (unsigned s = 0; s < sweeps; ++s) {
        launch(gp_points, track_blocks, in, sc, rule_of(s));
        launch(gp_cameras, n_images, in, sc, rule_of(s));
        launch(gp_gauge, 1u, in, sc, rule_of(s), s, trace, counts);
    }
    // the final weights follow the last sweep's rule (unit weights without a sweep)
    const GpRule last = sweeps ? rule_of(sweeps - 1) : GpRule{s0, min_obs, false};
    launch(gp_final_images, n_images, in, sc, last, poses_out, image_stats, counts);
    launch(gp_final_tracks, track_blocks, in, sc, last, points_out, obs_state, counts);
    return issued;
}

}  // namespace lfmkd
