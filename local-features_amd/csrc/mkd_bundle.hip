// gfx950 bundle adjustment (include/lf_mkd.h, lf_mkd_bundle_adjust_device): Levenberg-Marquardt on the
// reprojection error over the free cameras (6 parameters each) and the free points of a track table, the reduced camera system
// solved matrix-free by conjugate gradients preconditioned with the damped camera blocks.  The arithmetic is
// csrc/mkd_bundle_math.h, which the host twin compiles too.  Every launch is sized on the host from the call's arguments
// alone; T, O, the ranges, lambda, the CG scalars and the accepted state's index are read on the device, so the sequence is
// the same whatever the data hold (a stopped CG step and a rejected LM step are launches that do nothing).
//
// Two shapes of kernel, the two orders the sums run in:
//   per TRACK   4 lanes own a track (16 tracks a wave) as in mkd_triangulate.hip: lane l reads the positions lo + l, lo + 4 + l,
//               .. in ascending order, so the lane IS the slot of the 4-slot canonical sum; the butterfly over lane xor 2, 1.
//   per IMAGE   a workgroup of 256 owns an image as in mkd_resect.hip: thread s reads entries s, s + 256, .. of the image's
//               ascending list of active rows, so the thread IS the slot of the 256-slot canonical sum.
// and ONE workgroup for every global sum (over image id, or over track index, in the 256-slot order) and the scalars.
//
//   ba_init, ba_setup_tracks, ba_setup_images   the f64 state, the flags, the ACTIVE set, the inverse map row -> (position,
//               track) and every image's list, compacted in ascending order as rs_gather's
//   per LM iteration:
//     ba_track_lin    V, g_p and the cost of every track at the state; the damped V*, HELD points, y = V*^-1 g_p
//     ba_image_lin    U, g_c of every free image; the damped U*, HELD cameras; which observations are coupled;
//                     b = g_c - sum W y, and the start of CG: r = b, z = U*^-1 r, p = z, x = 0, r.z
//     ba_scalar       (start) cost_k and r.z summed
//     per CG step: ba_track_apply (y = V*^-1 sum W^T p), ba_image_apply (Ap = U* p - sum W y, p.Ap), ba_scalar (alpha),
//                  ba_cg_update (x, r, z, r.z), ba_scalar (beta, and p = z + beta p)
//     ba_cam_step     the candidate cameras rs_update(x)
//     ba_track_step   dp = V*^-1 (g_p - sum W^T x), the candidate points, the candidate's cost per track
//     ba_scalar       (accept) cost' summed, the verdict, lambda, the trace row; the state is two buffers and an index
//   ba_final_images, ba_final_tracks   the rounding, the copies, the states, the counts
//
// W is RECOMPUTED at every use from the keypoint, the point and the pose (one division chain, 18 products) rather than stored
// per observation (144 bytes written once and read twice a CG step): measured, recomputing is 11 % faster on a collection of
// 128 000 observations and 5 % on a window of 256 000, equal on a single query image, the same bits, and the scratch is 4
// bytes a position instead of 148 (profiles/bundle.md; -DLF_BA_STORE_W builds the other form).  One image owning every row
// serialises the per-image kernels on one workgroup: its passes are M / 256 rounds of one workgroup, the cost stated in
// the header and measured in profiles/bundle.md.
//
// lf_mkd_bundle_adjust_intrinsics_device is the SAME kernels instantiated with kI = true: the intrinsics an
// observation is read under are then doubles, the f32 input widened or, for an image of a free group, the products of the
// group's state (s, dx, dy); the per-image kernels also walk the usable images that are not free but inform a free group, and
// gather the group's own terms, the block U_ck between camera and group and, per CG step, the image's share of the group's
// operator row; ba_setup_groups, ba_group_lin and ba_group_apply (a workgroup per group, walking every image id in the
// 256-slot order: n_groups x n_images reads a CG step, the cost stated in the header) sum those shares, and the thread-per-
// image kernels take the groups as further threads.  With nothing refined no group is free and every shared word is the
// fixed-intrinsics call's.
//
// No floating-point atomic (the integer counts of the trace are integer atomics, exact in any order), no LDS beyond the block
// sums, scratch belongs to the handle, nobody waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mkd_bundle_math.h"
#include "mkd_device.h"
#include "mkd_scene.h"

namespace lfmkd {
namespace {

constexpr int kThreads = kRsSlots;
constexpr int kWaves = kThreads / 64;
constexpr int G = 4;
static_assert(kThreads == kSumThreads && kTriSlots == G, "thread s is slot s of the 256-slot sum, lane l slot l of the 4-slot sum");
constexpr unsigned kMaxBlocks = 16384;      // grid-stride beyond

enum : int { kVecX = 0, kVecR = 1, kVecZ = 2, kVecP = 3, kVecAp = 4, kVecs = 5 };
enum : int { kSLambda = 0, kSCost = 1, kSRz = 2, kSRz0 = 3, kSAlpha = 4, kSBeta = 5, kScalars = 8 };
enum : int { kWCur = 0, kWStopped = 1, kWSteps = 2, kWInliers = 3, kWHeldCams = 4, kWHeldPoints = 5, kWFreeCams = 6,
             kWFreePoints = 7, kWActive = 8, kWAccepted = 9, kWHeldGroups = 10, kWFreeGroups = 11, kWBadSigma = 12, kWords = 16 };
enum : unsigned { kModeStart = 0, kModeAlpha = 1, kModeBeta = 2, kModeAccept = 3 };

// scratch, in bundle_scratch_bytes' order: the f64 arrays, the 64-bit map, then the words
struct BaScratch {
    RsPose *cam;                 // [2][n_images]: the state and the candidate, words[kWCur] says which is which
    double *pt;                  // [2][tcap][3]
    double *U;                   // [n_images][27]: damped U*, then g_c
    double *V;                   // [tcap][9]: damped V*, then g_p
    double *W;                   // [ocap][18] in the A/B build that stores W; not allocated otherwise
    double *vec;                 // [5][n_images][6]: x, r, z, p, Ap
    double *y;                   // [tcap][3]
    double *tcost;               // [tcap]
    double *dots;                // [n_images]
    double *scal;                // [kScalars]
    unsigned long long *rowmap;  // [n_rows]: position | track << 32 of the active observation that names the row
    unsigned *idx;               // [n_rows]: image i's active rows at [lo_i, lo_i + M_i)
    unsigned *head;              // [n_images][2] = {M, flags}
    unsigned *oflag;             // [ocap]
    unsigned *tflag;             // [tcap]
    unsigned *words;             // [kWords]
};

// What the intrinsics call adds: its arguments and, behind the scratch above, its own (nothing of it is read when kI is false)
struct BaIntr {
    const unsigned *__restrict__ group;        // may be null: every image is in group 0
    unsigned n_groups, refine;
    BaGroup *gstate;             // [2][n_groups]: the state and the candidate, as cam
    double *gU;                  // [n_groups][9]: damped U_kk*, then g_k
    double *gvec;                // [5][n_groups][3]: x, r, z, p, Ap
    double *gdots;               // [n_groups]
    double *Uck;                 // [n_images][18]
    double *ipart;               // [n_images][12]: an image's share of its group's sums (ba_image_lin: the nine terms and sum W_k y;
                                 // ba_image_apply: U_ck^T p_c - sum W_k y in the first three)
    unsigned *icount;            // [n_images]: the image's inliers
    unsigned *gflag;             // [n_groups]
};
template <bool kI>
using KOf = std::conditional_t<kI, double, float>;

__device__ __forceinline__ double *vec_of(const BaScratch &sc, const SceneTables &in, int which, unsigned img) {
    return sc.vec + ((uint64_t)which * in.n_images + img) * 6;
}
__device__ __forceinline__ void load_k0(const SceneTables &in, unsigned img, float *K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];
}
__device__ __forceinline__ double *gvec_of(const BaIntr &gi, int which, unsigned g) {
    return gi.gvec + ((uint64_t)which * gi.n_groups + g) * 3;
}
__device__ __forceinline__ unsigned group_of(const BaIntr &gi, unsigned img) { return gi.group ? gi.group[img] : 0u; }
__device__ __forceinline__ bool group_free(const BaIntr &gi, unsigned g) { return g < gi.n_groups && (gi.gflag[g] & kBaGroupFree); }
__device__ __forceinline__ bool group_moves(const BaIntr &gi, unsigned g) {
    return g < gi.n_groups && (gi.gflag[g] & (kBaGroupFree | kBaGroupHeld)) == kBaGroupFree;
}
// the intrinsics an image is read under: the input, or (kI) doubles -- the input widened, or for an image of a free group the
// products of the group's state `st` (words[kWCur], or the other one for the candidate)
template <bool kI>
__device__ __forceinline__ void load_k(const SceneTables &in, const BaIntr &gi, unsigned st, unsigned img, KOf<kI> *K) {
    if constexpr (!kI) {
        load_k0(in, img, K);
    } else {
        float K0[4];
        load_k0(in, img, K0);
        ba_widen_k(K0, K);
        const unsigned g = group_of(gi, img);
        if (group_free(gi, g)) ba_group_k(K0, gi.gstate[(uint64_t)st * gi.n_groups + g], K);
    }
}
// the correspondence of an ACTIVE position's row under the points `pt`
__device__ __forceinline__ BaCorr load_corr(const SceneTables &in, uint64_t row, const double *pt, uint64_t t) {
    const float *k = in.kps + 5 * row;
    const double *p = pt + 3 * t;
    return BaCorr{k[0], k[1], p[0], p[1], p[2]};
}

// The coupling block of a coupled position, formed again from the state at every use (the state does not move within an
// iteration, so these are ba_image_lin's bits), or -- the A/B build of profiles/bundle.md, -DLF_BA_STORE_W -- as ba_image_lin
// stored it, 144 bytes a position.
__device__ __forceinline__ void load_w(const SceneTables &in, const BaScratch &sc, uint64_t pos, uint64_t t, double *W) {
#ifndef LF_BA_STORE_W
    const unsigned cur = sc.words[kWCur], img = in.obs_image[pos];
    float K[4];
    load_k0(in, img, K);
    BaLin o;
    ba_rows(sc.cam[(uint64_t)cur * in.n_images + img], K,
            load_corr(in, (uint64_t)in.obs_row[pos], sc.pt + (uint64_t)cur * in.tcap * 3, t), o);
    ba_coupling(o, W);
#else
    const double *src = sc.W + kBaW * pos;
#pragma unroll
    for (int i = 0; i < kBaW; ++i) W[i] = src[i];
#endif
}

// (kI) the rows of a position at the state, from which both its coupling blocks are formed, and its image's input intrinsics
__device__ __forceinline__ void load_lin(const SceneTables &in, const BaIntr &gi, const BaScratch &sc, uint64_t pos, uint64_t t, BaLin &o,
                                         float *K0) {
    const unsigned cur = sc.words[kWCur], img = in.obs_image[pos];
    double K[4];
    load_k<true>(in, gi, cur, img, K);
    load_k0(in, img, K0);
    ba_rows(sc.cam[(uint64_t)cur * in.n_images + img], K,
            load_corr(in, (uint64_t)in.obs_row[pos], sc.pt + (uint64_t)cur * in.tcap * 3, t), o);
}
// what a coupled or group-coupled position adds to sum W^T v over its track: W_c^T v_c + W_k^T v_k, or the one that enters (v = p
// or x)
__device__ __forceinline__ void add_wt(const SceneTables &in, const BaIntr &gi, const BaScratch &sc, uint64_t pos, uint64_t t, int which,
                                       double *acc) {
    const unsigned of = sc.oflag[pos];
    if (!(of & (kBaCoupled | kBaInlier))) return;
    const unsigned img = in.obs_image[pos], g = group_of(gi, img);
    const bool kc = (of & kBaInlier) && group_moves(gi, g);
    if (!(of & kBaCoupled) && !kc) return;
    BaLin o;
    float K0[4];
    load_lin(in, gi, sc, pos, t, o, K0);
    double w[3] = {0.0, 0.0, 0.0};
    if (of & kBaCoupled) {
        double W[kBaW];
        ba_coupling(o, W);
        ba_wt_v(W, vec_of(sc, in, which, img), w);
    }
    if (kc) {
        BaGRows gr;
        double W[kBaWk], v[3];
        ba_group_rows(o, K0, gi.refine, gr);
        ba_coupling_k(o, gr, W);
        ba_wkt_v(W, gvec_of(gi, which, g), v);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = (of & kBaCoupled) ? w[k] + v[k] : v[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + w[k];
}

}  // namespace

// ---- setup ------------------------------------------------------------------------------------------------------------------------
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_init(SceneTables in, BaIntr gi, const float *__restrict__ poses,
                                                    const unsigned *__restrict__ fixed, double lambda0, BaScratch sc) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, n = (uint64_t)gridDim.x * kThreads;
    for (uint64_t r = gid; r < in.n_rows; r += n) sc.rowmap[r] = kBaNoRow;
    for (uint64_t i = gid; i < in.n_images; i += n) {
        float K[4], P[12];
        load_k0(in, (unsigned)i, K);
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = poses[12 * i + k];
        const bool usable = tri_camera_usable(K, P), is_free = usable && !(fixed && fixed[i] != 0);
        sc.head[2 * i] = 0;
        sc.head[2 * i + 1] = (usable ? kBaCamUsable : 0u) | (is_free ? kBaCamFree : 0u);
        RsPose S;
#pragma unroll
        for (int k = 0; k < 9; ++k) S.R[k] = double(P[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) S.t[k] = double(P[9 + k]);
        sc.cam[i] = S;
        sc.cam[in.n_images + i] = S;
    }
    if constexpr (kI)
        for (uint64_t g = gid; g < gi.n_groups; g += n) {
            gi.gstate[g] = gi.gstate[gi.n_groups + g] = BaGroup{1.0, 0.0, 0.0};
            gi.gflag[g] = 0;
        }
    if (gid < kWords) sc.words[gid] = 0;
    if (gid < kScalars) sc.scal[gid] = gid == kSLambda ? lambda0 : 0.0;
}

__global__ __launch_bounds__(kThreads) void ba_setup_tracks(SceneTables in, const float *__restrict__ points,
                                                            const unsigned *__restrict__ obs_state, BaScratch sc) {
    const TrackWalk w = track_walk(in);
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < w.T;
        uint64_t lo = 0, hi = 0;
        bool ok = false;
        double X[3] = {0.0, 0.0, 0.0};
        if (alive) {
            track_range(in, t, w.O, lo, hi);
            const float p[4] = {points[4 * t], points[4 * t + 1], points[4 * t + 2], points[4 * t + 3]};
            ok = rs_point_usable(p, 1.0);
#pragma unroll
            for (int k = 0; k < 3; ++k) X[k] = double(p[k]);
        }
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);
        unsigned n_active = 0;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            const bool in_track = ch < nch && pos < hi;
            bool act = false;
            if (in_track) {
                const int row = in.obs_row[pos];
                const unsigned img = in.obs_image[pos];
                if (ok && row >= 0 && (uint64_t)row < in.n_rows && img < in.n_images && (sc.head[2 * (uint64_t)img + 1] & kBaCamUsable) &&
                    (!obs_state || obs_state[pos] == 2u)) {
                    uint64_t ilo, ihi;
                    image_range(in, img, ilo, ihi);
                    const float *k = in.kps + 5 * (uint64_t)row;
                    act = (uint64_t)row >= ilo && (uint64_t)row < ihi && tri_keypoint_usable(k[0], k[1]);
                    if (act) sc.rowmap[row] = (unsigned long long)pos | (unsigned long long)t << 32;
                }
                sc.oflag[pos] = act ? kBaActive : 0u;
            }
            n_active += (unsigned)__popc(group_bits(act, w.base));
        }
        if (alive && w.l == 0) {
            sc.tflag[t] = (ok ? kBaPointOk : 0u) | (n_active ? kBaPointFree : 0u);
#pragma unroll
            for (int k = 0; k < 3; ++k) sc.pt[3 * t + k] = X[k], sc.pt[3 * (in.tcap + t) + k] = X[k];
            if (n_active) atomicAdd(sc.words + kWFreePoints, 1u), atomicAdd(sc.words + kWActive, n_active);
        }
    }
}

// (kI: a list for every usable image, since a camera that is not free still informs its group)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_setup_images(SceneTables in, BaScratch sc) {
    __shared__ unsigned s_cnt[kWaves];
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    const unsigned hf0 = sc.head[2 * (uint64_t)img + 1];
    if (!(hf0 & (kI ? kBaCamUsable : kBaCamFree))) return;                        // block-uniform; M stays 0
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    uint64_t base = lo;
    for (uint64_t r0 = lo; r0 < hi; r0 += kThreads) {                             // block-uniform
        const uint64_t r = r0 + tid;
        bool is = false;
        if (r < hi) {
            const unsigned long long m = sc.rowmap[r];
            is = m != kBaNoRow && in.obs_image[(unsigned)m] == img;
        }
        block_compact(is, (unsigned)r, sc.idx, s_cnt, base);
    }
    if (tid == 0) {
        sc.head[2 * (uint64_t)img] = (unsigned)(base - lo);
        if (hf0 & kBaCamFree) atomicAdd(sc.words + kWFreeCams, 1u);
    }
}

// a workgroup per group: FREE iff something is refined and a usable image of the group has an active row
__global__ __launch_bounds__(kThreads) void ba_setup_groups(SceneTables in, BaIntr gi, BaScratch sc) {
    const unsigned g = blockIdx.x;
    int found = 0;
    for (uint64_t i = threadIdx.x; i < in.n_images; i += kThreads)
        found |= group_of(gi, (unsigned)i) == g && (sc.head[2 * i + 1] & kBaCamUsable) && sc.head[2 * i] != 0;
    found = __syncthreads_or(found);
    if (threadIdx.x == 0 && gi.refine && found) {
        gi.gflag[g] = kBaGroupFree;
        atomicAdd(sc.words + kWFreeGroups, 1u);
    }
}

// ---- an LM iteration -------------------------------------------------------------------------------------------------------------
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_track_lin(SceneTables in, BaIntr gi, double thr2, BaScratch sc) {
    const TrackWalk w = track_walk(in);
    const unsigned cur = sc.words[kWCur];
    const double lambda = sc.scal[kSLambda];
    const RsPose *cam = sc.cam + (uint64_t)cur * in.n_images;
    const double *pt = sc.pt + (uint64_t)cur * in.tcap * 3;
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < w.T;
        uint64_t lo = 0, hi = 0;
        if (alive) track_range(in, t, w.O, lo, hi);
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);
        double acc[kBaPointTerms + 1];
#pragma unroll
        for (int k = 0; k <= kBaPointTerms; ++k) acc[k] = 0.0;
        unsigned n_in = 0;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            const bool on = ch < nch && pos < hi && (sc.oflag[pos] & kBaActive);
            bool inl = false;
            if (on) {
                const unsigned img = in.obs_image[pos];
                KOf<kI> K[4];
                load_k<kI>(in, gi, cur, img, K);
                BaLin o;
                ba_linearise(cam[img], K, load_corr(in, (uint64_t)in.obs_row[pos], pt, t), thr2, o);
                inl = o.inlier;
                acc[kBaPointTerms] = acc[kBaPointTerms] + (inl ? o.e2 : thr2);
                if (inl) {
                    double v[kBaPointTerms];
                    ba_point_terms(o, v);
#pragma unroll
                    for (int k = 0; k < kBaPointTerms; ++k) acc[k] = acc[k] + v[k];
                }
            }
            n_in += (unsigned)__popc(group_bits(inl, w.base));
        }
        double v[kBaPointTerms], y[3];
#pragma unroll
        for (int k = 0; k < kBaPointTerms; ++k) v[k] = combine(acc[k]);
        const double cost = combine(acc[kBaPointTerms]);
        ba_damp_v(v, lambda);
        const bool ok = ba_solve_v(v, v + 6, y);
        if (alive && w.l == 0) {
            const unsigned tf = sc.tflag[t] & (kBaPointOk | kBaPointFree);
            const bool is_free = (tf & kBaPointFree) != 0, held = is_free && (n_in < 2 || !ok);
            sc.tflag[t] = tf | (held ? kBaPointHeld : 0u);
            sc.tcost[t] = cost;
#pragma unroll
            for (int k = 0; k < kBaPointTerms; ++k) sc.V[kBaPointTerms * t + k] = v[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) sc.y[3 * t + k] = is_free && !held ? y[k] : 0.0;
            if (n_in) atomicAdd(sc.words + kWInliers, n_in);
            if (held) atomicAdd(sc.words + kWHeldPoints, 1u);
        }
    }
}

template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_image_lin(SceneTables in, BaIntr gi, double thr2, BaScratch sc) {
    __shared__ double s_red[kWaves * kRsTerms];
    __shared__ unsigned s_cnt;
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    const unsigned hf = sc.head[2 * (uint64_t)img + 1] & (kBaCamUsable | kBaCamFree);
    const bool is_free = (hf & kBaCamFree) != 0;
    bool informs = false;                                                         // (kI) a usable image of a free group
    if constexpr (kI) informs = (hf & kBaCamUsable) && group_free(gi, group_of(gi, img));
    if (!is_free) {                                                               // block-uniform
        if (tid < 6) {
#pragma unroll
            for (int k = 0; k < kVecs; ++k) vec_of(sc, in, k, img)[tid] = 0.0;
        }
        if (tid == 0) sc.dots[img] = 0.0;
        if (!informs) return;
    }
    const unsigned cur = sc.words[kWCur], M = sc.head[2 * (uint64_t)img];
    const double lambda = sc.scal[kSLambda];
    const RsPose P = sc.cam[(uint64_t)cur * in.n_images + img];
    const double *pt = sc.pt + (uint64_t)cur * in.tcap * 3;
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    KOf<kI> K[4];
    load_k<kI>(in, gi, cur, img, K);
    float K0[4];
    load_k0(in, img, K0);

    if constexpr (kI) {
        // the image's share of its group's sums: the nine terms, its inliers, and U_ck (block-uniform)
        if (informs) {
            double ga[kBaGroupTerms + kBaCk];
#pragma unroll
            for (int i = 0; i < kBaGroupTerms + kBaCk; ++i) ga[i] = 0.0;
            unsigned n_in = 0;
            for (unsigned k = tid; k < M; k += kThreads) {
                const unsigned row = sc.idx[lo + k];
                const unsigned long long m = sc.rowmap[row];
                BaLin o;
                ba_linearise(P, K, load_corr(in, row, pt, m >> 32), thr2, o);
                if (o.inlier) {
                    BaGRows gr;
                    double v[kBaGroupTerms + kBaCk];
                    ba_group_rows(o, K0, gi.refine, gr);
                    ba_group_terms(o, gr, v);
                    ba_cross(o, gr, v + kBaGroupTerms);
#pragma unroll
                    for (int i = 0; i < kBaGroupTerms + kBaCk; ++i) ga[i] = ga[i] + v[i];
                    ++n_in;
                }
            }
            block_sum<double, kBaGroupTerms + kBaCk>(ga, s_red);
            n_in = block_count(n_in, &s_cnt);
            if (tid < kBaGroupTerms + kBaCk) {
                double v = ga[0];
#pragma unroll
                for (int i = 1; i < kBaGroupTerms + kBaCk; ++i) v = tid == (unsigned)i ? ga[i] : v;
                if (tid < kBaGroupTerms) gi.ipart[12 * (uint64_t)img + tid] = v;
                else gi.Uck[(uint64_t)kBaCk * img + (tid - kBaGroupTerms)] = v;
            }
            if (tid == 0) gi.icount[img] = n_in;
        }
    }

    double acc[kRsTerms];
#pragma unroll
    for (int i = 0; i < kRsTerms; ++i) acc[i] = 0.0;
    for (unsigned k = tid; k < (is_free ? M : 0u); k += kThreads) {               // (a camera that is not free has no block)
        const unsigned row = sc.idx[lo + k];
        const unsigned long long m = sc.rowmap[row];
        BaLin o;
        ba_linearise(P, K, load_corr(in, row, pt, m >> 32), thr2, o);
        if (o.inlier) {
            double v[kRsTerms];
            rs_gn_products(o.r, v);
#pragma unroll
            for (int i = 0; i < kRsTerms; ++i) acc[i] = acc[i] + v[i];
        }
    }
    block_sum<double, kRsTerms>(acc, s_red);
    ba_damp_u(acc, lambda);
    double z[6];
    const bool held = !ba_solve_u(acc, acc + 21, z) || !is_free;                  // every thread the same bits
    if (tid == 0 && is_free) {
        sc.head[2 * (uint64_t)img + 1] = hf | (held ? kBaCamHeld : 0u);
        if (held) atomicAdd(sc.words + kWHeldCams, 1u);
    }
    if (tid < kRsTerms && is_free) {
        double v = acc[0];
#pragma unroll
        for (int i = 1; i < kRsTerms; ++i) v = tid == (unsigned)i ? acc[i] : v;
        sc.U[(uint64_t)kRsTerms * img + tid] = v;
    }

    // which entries are coupled, and sum W y (kI: and sum W_k y over the inliers whose point moves)
    double s[kI ? 9 : 6];
#pragma unroll
    for (int i = 0; i < (kI ? 9 : 6); ++i) s[i] = 0.0;
    for (unsigned k = tid; k < M; k += kThreads) {
        const unsigned row = sc.idx[lo + k];
        const unsigned long long m = sc.rowmap[row];
        const uint64_t pos = (unsigned)m, t = m >> 32;
        BaLin o;
        ba_linearise(P, K, load_corr(in, row, pt, t), thr2, o);
        const bool coupled = !held && o.inlier && (sc.tflag[t] & (kBaPointFree | kBaPointHeld)) == kBaPointFree;
        if (coupled) {
            double W[kBaW], wy[6];
            ba_coupling(o, W);
#ifdef LF_BA_STORE_W
            double *dst = sc.W + kBaW * pos;
#pragma unroll
            for (int i = 0; i < kBaW; ++i) dst[i] = W[i];
#endif
            ba_w_y(W, sc.y + 3 * t, wy);
#pragma unroll
            for (int i = 0; i < 6; ++i) s[i] = s[i] + wy[i];
        }
        if constexpr (kI) {
            if (informs && o.inlier && (sc.tflag[t] & (kBaPointFree | kBaPointHeld)) == kBaPointFree) {
                BaGRows gr;
                double W[kBaWk], wy[3];
                ba_group_rows(o, K0, gi.refine, gr);
                ba_coupling_k(o, gr, W);
                ba_wk_y(W, sc.y + 3 * t, wy);
#pragma unroll
                for (int i = 0; i < 3; ++i) s[6 + i] = s[6 + i] + wy[i];
            }
            sc.oflag[pos] = kBaActive | (coupled ? kBaCoupled : 0u) | (o.inlier ? kBaInlier : 0u);
        } else {
            sc.oflag[pos] = kBaActive | (coupled ? kBaCoupled : 0u);
        }
    }
    block_sum<double, kI ? 9 : 6>(s, s_red);
    if constexpr (kI) {
        if (tid == 0 && informs) {
#pragma unroll
            for (int i = 0; i < 3; ++i) gi.ipart[12 * (uint64_t)img + 9 + i] = s[6 + i];
        }
    }
    if (tid == 0 && is_free) {
        double r[6], zz[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) r[i] = held ? 0.0 : acc[21 + i] - s[i];
        const bool ok = ba_solve_u(acc, r, zz);
        (void)ok;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double zi = held ? 0.0 : zz[i];
            vec_of(sc, in, kVecX, img)[i] = 0.0;
            vec_of(sc, in, kVecR, img)[i] = r[i];
            vec_of(sc, in, kVecZ, img)[i] = zi;
            vec_of(sc, in, kVecP, img)[i] = zi;
            vec_of(sc, in, kVecAp, img)[i] = 0.0;
            zz[i] = zi;
        }
        sc.dots[img] = held ? 0.0 : ba_dot6(r, zz);
    }
}

// A workgroup per group: the group's nine sums and its inliers over the shares of its usable images (slot = image id mod 256),
// the damped block, HELD, b_k = g_k - sum W_k y, and the start of CG for the group's three.
__global__ __launch_bounds__(kThreads) void ba_group_lin(SceneTables in, BaIntr gi, BaScratch sc) {
    __shared__ double s_red[kWaves * 12];
    __shared__ unsigned s_cnt;
    const unsigned g = blockIdx.x, tid = threadIdx.x;
    if (!(gi.gflag[g] & kBaGroupFree)) {                                          // block-uniform
        if (tid < 3) {
#pragma unroll
            for (int k = 0; k < kVecs; ++k) gvec_of(gi, k, g)[tid] = 0.0;
        }
        if (tid == 0) gi.gdots[g] = 0.0;
        return;
    }
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    unsigned n_in = 0;
    for (uint64_t i = tid; i < in.n_images; i += kThreads)
        if (group_of(gi, (unsigned)i) == g && (sc.head[2 * i + 1] & kBaCamUsable)) {
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[k] = acc[k] + gi.ipart[12 * i + k];
            n_in += gi.icount[i];
        }
    block_sum<double, 12>(acc, s_red);
    n_in = block_count(n_in, &s_cnt);
    ba_group_block(acc, sc.scal[kSLambda], gi.refine);
    double z[3];
    const bool held = !ba_solve_v(acc, acc + 6, z) || n_in == 0;                  // every thread the same bits
    if (tid != 0) return;
    gi.gflag[g] = kBaGroupFree | (held ? kBaGroupHeld : 0u);
    if (held) atomicAdd(sc.words + kWHeldGroups, 1u);
    double r[3], zz[3];
#pragma unroll
    for (int k = 0; k < kBaGroupTerms; ++k) gi.gU[(uint64_t)kBaGroupTerms * g + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = held ? 0.0 : acc[6 + k] - acc[9 + k];
    ba_group_mask(r, gi.refine);
    ba_solve_v(acc, r, zz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double zk = held ? 0.0 : zz[k];
        gvec_of(gi, kVecX, g)[k] = 0.0;
        gvec_of(gi, kVecR, g)[k] = r[k];
        gvec_of(gi, kVecZ, g)[k] = zk;
        gvec_of(gi, kVecP, g)[k] = zk;
        gvec_of(gi, kVecAp, g)[k] = 0.0;
        zz[k] = zk;
    }
    gi.gdots[g] = held ? 0.0 : ba_dot3(r, zz);
}

// y = V*^-1 sum W^T p over the track's coupled positions (0 for a point that is not free, or held)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_track_apply(SceneTables in, BaIntr gi, BaScratch sc) {
    if (sc.words[kWStopped]) return;                                              // grid-uniform
    const TrackWalk w = track_walk(in);
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool go = t < w.T && (sc.tflag[t] & (kBaPointFree | kBaPointHeld)) == kBaPointFree;
        uint64_t lo = 0, hi = 0;
        if (go) track_range(in, t, w.O, lo, hi);
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);
        double acc[3] = {0.0, 0.0, 0.0};
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            if constexpr (kI) {
                if (ch < nch && pos < hi) add_wt(in, gi, sc, pos, t, kVecP, acc);
            } else if (ch < nch && pos < hi && (sc.oflag[pos] & kBaCoupled)) {
                double W[kBaW], v[3];
                load_w(in, sc, pos, t, W);
                ba_wt_v(W, vec_of(sc, in, kVecP, in.obs_image[pos]), v);
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[k] = acc[k] + v[k];
            }
        }
        double b[3], y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = combine(acc[k]);
        if (go) ba_solve_v(sc.V + kBaPointTerms * t, b, y);
        if (go && w.l == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sc.y[3 * t + k] = y[k];
        }
    }
}

// Ap = U* p - sum W y over the image's coupled entries, and p.Ap
// (kI, the image's group moving: Ap = (U* p + U_ck p_k) - sum W y, and the image's share U_ck^T p - sum W_k y of the group's row)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_image_apply(SceneTables in, BaIntr gi, BaScratch sc) {
    __shared__ double s_red[kWaves * 9];
    if (sc.words[kWStopped]) return;                                              // grid-uniform
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    const unsigned hf = sc.head[2 * (uint64_t)img + 1];
    const bool moves = (hf & (kBaCamFree | kBaCamHeld)) == kBaCamFree;
    unsigned g = 0;
    bool gmoves = false;                                                          // (kI) a usable image of a moving group
    if constexpr (kI) {
        g = group_of(gi, img);
        gmoves = (hf & kBaCamUsable) && group_moves(gi, g);
    }
    if (!moves) {                                                                 // block-uniform
        if (tid == 0) sc.dots[img] = 0.0;
        if (!gmoves) return;
    }
    const unsigned M = sc.head[2 * (uint64_t)img];
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    double s[kI ? 9 : 6];
#pragma unroll
    for (int i = 0; i < (kI ? 9 : 6); ++i) s[i] = 0.0;
    for (unsigned k = tid; k < M; k += kThreads) {
        const unsigned long long m = sc.rowmap[sc.idx[lo + k]];
        const uint64_t pos = (unsigned)m, t = m >> 32;
        if constexpr (kI) {
            const unsigned of = sc.oflag[pos];
            const bool kc = gmoves && (of & kBaInlier) && (sc.tflag[t] & (kBaPointFree | kBaPointHeld)) == kBaPointFree;
            if ((of & kBaCoupled) || kc) {
                BaLin o;
                float K0[4];
                load_lin(in, gi, sc, pos, t, o, K0);
                if (of & kBaCoupled) {
                    double W[kBaW], wy[6];
                    ba_coupling(o, W);
                    ba_w_y(W, sc.y + 3 * t, wy);
#pragma unroll
                    for (int i = 0; i < 6; ++i) s[i] = s[i] + wy[i];
                }
                if (kc) {
                    BaGRows gr;
                    double W[kBaWk], wy[3];
                    ba_group_rows(o, K0, gi.refine, gr);
                    ba_coupling_k(o, gr, W);
                    ba_wk_y(W, sc.y + 3 * t, wy);
#pragma unroll
                    for (int i = 0; i < 3; ++i) s[6 + i] = s[6 + i] + wy[i];
                }
            }
        } else if (sc.oflag[pos] & kBaCoupled) {
            double W[kBaW], wy[6];
            load_w(in, sc, pos, t, W);
            ba_w_y(W, sc.y + 3 * t, wy);
#pragma unroll
            for (int i = 0; i < 6; ++i) s[i] = s[i] + wy[i];
        }
    }
    block_sum<double, kI ? 9 : 6>(s, s_red);
    if (tid == 0) {
        double p[6], up[6], ap[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) p[i] = vec_of(sc, in, kVecP, img)[i];
        if (moves) {
            ba_u_times(sc.U + (uint64_t)kRsTerms * img, p, up);
            if constexpr (kI) {
                if (gmoves) {
                    double ck[6];
                    ba_w_y(gi.Uck + (uint64_t)kBaCk * img, gvec_of(gi, kVecP, g), ck);
#pragma unroll
                    for (int i = 0; i < 6; ++i) up[i] = up[i] + ck[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                ap[i] = up[i] - s[i];
                vec_of(sc, in, kVecAp, img)[i] = ap[i];
            }
            sc.dots[img] = ba_dot6(p, ap);
        }
        if constexpr (kI) {
            if (gmoves) {
                double part[3] = {0.0, 0.0, 0.0};
                if (moves) ba_wt_v(gi.Uck + (uint64_t)kBaCk * img, p, part);
#pragma unroll
                for (int i = 0; i < 3; ++i) gi.ipart[12 * (uint64_t)img + i] = part[i] - s[6 + i];
            }
        }
    }
}

// A workgroup per moving group: Ap_k = U_kk* p_k + the sum over its usable images' shares (slot = image id mod 256), and p_k.Ap_k
__global__ __launch_bounds__(kThreads) void ba_group_apply(SceneTables in, BaIntr gi, BaScratch sc) {
    __shared__ double s_red[kWaves * 3];
    if (sc.words[kWStopped]) return;                                              // grid-uniform
    const unsigned g = blockIdx.x, tid = threadIdx.x;
    if (!group_moves(gi, g)) {                                                    // block-uniform
        if (tid == 0) gi.gdots[g] = 0.0;
        return;
    }
    double s[3] = {0.0, 0.0, 0.0};
    for (uint64_t i = tid; i < in.n_images; i += kThreads)
        if (group_of(gi, (unsigned)i) == g && (sc.head[2 * i + 1] & kBaCamUsable)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = s[k] + gi.ipart[12 * i + k];
        }
    block_sum<double, 3>(s, s_red);
    if (tid == 0) {
        double p[3], up[3], ap[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = gvec_of(gi, kVecP, g)[k];
        ba_v_times(gi.gU + (uint64_t)kBaGroupTerms * g, p, up);
#pragma unroll
        for (int k = 0; k < 3; ++k) ap[k] = up[k] + s[k];
        ba_group_mask(ap, gi.refine);
#pragma unroll
        for (int k = 0; k < 3; ++k) gvec_of(gi, kVecAp, g)[k] = ap[k];
        gi.gdots[g] = ba_dot3(p, ap);
    }
}

// x += alpha p, r -= alpha Ap, z = U*^-1 r, and r.z: a thread per image (kI: then a thread per group)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_cg_update(SceneTables in, BaIntr gi, BaScratch sc) {
    if (sc.words[kWStopped]) return;                                              // grid-uniform
    const uint64_t img = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if constexpr (kI) {
        if (img >= in.n_images && img - in.n_images < gi.n_groups) {
            const unsigned g = (unsigned)(img - in.n_images);
            if (!group_moves(gi, g)) {
                gi.gdots[g] = 0.0;
                return;
            }
            const double alpha = sc.scal[kSAlpha];
            double *x = gvec_of(gi, kVecX, g), *r = gvec_of(gi, kVecR, g);
            const double *p = gvec_of(gi, kVecP, g), *ap = gvec_of(gi, kVecAp, g);
            double rn[3], z[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                x[i] = x[i] + alpha * p[i];
                rn[i] = r[i] - alpha * ap[i];
                r[i] = rn[i];
            }
            ba_solve_v(gi.gU + (uint64_t)kBaGroupTerms * g, rn, z);
#pragma unroll
            for (int i = 0; i < 3; ++i) gvec_of(gi, kVecZ, g)[i] = z[i];
            gi.gdots[g] = ba_dot3(rn, z);
            return;
        }
    }
    if (img >= in.n_images) return;
    if ((sc.head[2 * img + 1] & (kBaCamFree | kBaCamHeld)) != kBaCamFree) {
        sc.dots[img] = 0.0;
        return;
    }
    const double alpha = sc.scal[kSAlpha];
    double *x = vec_of(sc, in, kVecX, (unsigned)img), *r = vec_of(sc, in, kVecR, (unsigned)img);
    const double *p = vec_of(sc, in, kVecP, (unsigned)img), *ap = vec_of(sc, in, kVecAp, (unsigned)img);
    double rn[6], z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        x[i] = x[i] + alpha * p[i];
        rn[i] = r[i] - alpha * ap[i];
        r[i] = rn[i];
    }
    ba_solve_u(sc.U + kRsTerms * img, rn, z);
#pragma unroll
    for (int i = 0; i < 6; ++i) vec_of(sc, in, kVecZ, (unsigned)img)[i] = z[i];
    sc.dots[img] = ba_dot6(rn, z);
}

// ONE workgroup: a global sum in the 256-slot order (over image id of dots, over track index of tcost) and the scalars
// (kI: a dot product is the 256-slot sum over the image ids plus the 256-slot sum over the group ids, in that order)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_scalar(SceneTables in, BaIntr gi, unsigned mode, double tol2, unsigned iteration, BaScratch sc,
                                                      double *__restrict__ trace) {
    constexpr int kSums = kI ? 3 : 2;
    __shared__ double s_red[kWaves * kSums];
    const unsigned tid = threadIdx.x;
    if ((mode == kModeAlpha || mode == kModeBeta) && sc.words[kWStopped]) return;
    const uint64_t T = clamp_to(in.counts[0], in.tcap);
    double v[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) v[i] = 0.0;
    if (mode != kModeAccept)
        for (uint64_t i = tid; i < in.n_images; i += kThreads) v[0] = v[0] + sc.dots[i];
    if (mode == kModeStart || mode == kModeAccept)
        for (uint64_t t = tid; t < T; t += kThreads) v[1] = v[1] + sc.tcost[t];
    if constexpr (kI) {
        if (mode != kModeAccept)
            for (uint64_t g = tid; g < gi.n_groups; g += kThreads) v[2] = v[2] + gi.gdots[g];
    }
    block_sum<double, kSums>(v, s_red);
    if constexpr (kI) v[0] = v[0] + v[2];
    BaCg cg = {sc.scal[kSRz], sc.scal[kSRz0], sc.scal[kSAlpha], sc.scal[kSBeta], sc.words[kWStopped], sc.words[kWSteps]};
    __syncthreads();                                                              // everyone has read the scalars
    if (mode == kModeStart) ba_cg_start(cg, v[0]);
    if (mode == kModeAlpha) ba_cg_alpha(cg, v[0]);
    if (mode == kModeBeta) {
        ba_cg_beta(cg, v[0], tol2);
        if (!cg.stopped)
            for (uint64_t i = tid; i < 6 * (uint64_t)in.n_images; i += kThreads) {
                double *p = sc.vec + (uint64_t)kVecP * in.n_images * 6, *z = sc.vec + (uint64_t)kVecZ * in.n_images * 6;
                p[i] = z[i] + cg.beta * p[i];
            }
        if constexpr (kI) {
            if (!cg.stopped)
                for (uint64_t i = tid; i < 3 * (uint64_t)gi.n_groups; i += kThreads) {
                    double *p = gi.gvec + (uint64_t)kVecP * gi.n_groups * 3, *z = gi.gvec + (uint64_t)kVecZ * gi.n_groups * 3;
                    p[i] = z[i] + cg.beta * p[i];
                }
        }
    }
    if (tid != 0) return;
    if (mode == kModeAccept) {
        double lambda = sc.scal[kSLambda];
        const double used = lambda, cost = sc.scal[kSCost];
        const bool ok = ba_accept(v[1], cost, lambda, !(kI && sc.words[kWBadSigma]));
        double *row = trace + (uint64_t)(kI ? kBaTraceI : kBaTrace) * iteration;
        row[0] = cost, row[1] = v[1], row[2] = used, row[3] = ok ? 1.0 : 0.0, row[4] = double(sc.words[kWSteps]);
        row[5] = double(sc.words[kWInliers]), row[6] = double(sc.words[kWHeldCams]), row[7] = double(sc.words[kWHeldPoints]);
        sc.scal[kSLambda] = lambda;
        if (ok) sc.words[kWCur] ^= 1u, sc.words[kWAccepted] += 1u;
        if constexpr (kI) row[8] = double(sc.words[kWHeldGroups]), sc.words[kWHeldGroups] = 0, sc.words[kWBadSigma] = 0;
        sc.words[kWInliers] = 0, sc.words[kWHeldCams] = 0, sc.words[kWHeldPoints] = 0;
        return;
    }
    if (mode == kModeStart) sc.scal[kSCost] = v[1];
    sc.scal[kSRz] = cg.rz, sc.scal[kSRz0] = cg.rz0, sc.scal[kSAlpha] = cg.alpha, sc.scal[kSBeta] = cg.beta;
    sc.words[kWStopped] = cg.stopped, sc.words[kWSteps] = cg.steps;
}

// the candidate cameras: a thread per image (kI: then the candidate groups, a thread per group; a moving group whose candidate s
// is not finite and positive marks the whole candidate as one to reject)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_cam_step(SceneTables in, BaIntr gi, BaScratch sc) {
    const uint64_t img = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const unsigned cur = sc.words[kWCur];
    if constexpr (kI) {
        if (img >= in.n_images && img - in.n_images < gi.n_groups) {
            const unsigned g = (unsigned)(img - in.n_images);
            const BaGroup S = gi.gstate[(uint64_t)cur * gi.n_groups + g];
            BaGroup next = S;
            if (group_moves(gi, g)) {
                double d[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) d[i] = gvec_of(gi, kVecX, g)[i];
                if (!ba_group_step(S, d, gi.refine, next)) atomicOr(sc.words + kWBadSigma, 1u);
            }
            gi.gstate[(uint64_t)(cur ^ 1u) * gi.n_groups + g] = next;
            return;
        }
    }
    if (img >= in.n_images) return;
    const RsPose P = sc.cam[(uint64_t)cur * in.n_images + img];
    RsPose next = P;
    if ((sc.head[2 * img + 1] & (kBaCamFree | kBaCamHeld)) == kBaCamFree) {
        double d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = vec_of(sc, in, kVecX, (unsigned)img)[i];
        rs_update(P, d, next);
    }
    sc.cam[(uint64_t)(cur ^ 1u) * in.n_images + img] = next;
}

// the candidate points X - V*^-1 (g_p - sum W^T x) and the candidate's cost per track
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_track_step(SceneTables in, BaIntr gi, double thr2, BaScratch sc) {
    const TrackWalk w = track_walk(in);
    const unsigned cur = sc.words[kWCur];
    const RsPose *cam_c = sc.cam + (uint64_t)(cur ^ 1u) * in.n_images;
    const double *pt = sc.pt + (uint64_t)cur * in.tcap * 3;
    double *pt_c = sc.pt + (uint64_t)(cur ^ 1u) * in.tcap * 3;
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < w.T;
        const bool go = alive && (sc.tflag[t] & (kBaPointFree | kBaPointHeld)) == kBaPointFree;
        uint64_t lo = 0, hi = 0;
        if (alive) track_range(in, t, w.O, lo, hi);
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);
        double acc[3] = {0.0, 0.0, 0.0};
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            if constexpr (kI) {
                if (go && ch < nch && pos < hi) add_wt(in, gi, sc, pos, t, kVecX, acc);
            } else if (go && ch < nch && pos < hi && (sc.oflag[pos] & kBaCoupled)) {
                double W[kBaW], v[3];
                load_w(in, sc, pos, t, W);
                ba_wt_v(W, vec_of(sc, in, kVecX, in.obs_image[pos]), v);
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[k] = acc[k] + v[k];
            }
        }
        BaCorr c = {0.f, 0.f, 0.0, 0.0, 0.0};
        if (alive) c.X = pt[3 * t], c.Y = pt[3 * t + 1], c.Z = pt[3 * t + 2];
        double b[3], dp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = combine(acc[k]);
        if (go) {
            const double *V = sc.V + kBaPointTerms * t;
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] = V[6 + k] - b[k];
            ba_solve_v(V, b, dp);
            c.X = c.X - dp[0], c.Y = c.Y - dp[1], c.Z = c.Z - dp[2];
        }
        double cost = 0.0;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            if (ch < nch && pos < hi && (sc.oflag[pos] & kBaActive)) {
                const unsigned img = in.obs_image[pos];
                KOf<kI> K[4];
                load_k<kI>(in, gi, cur ^ 1u, img, K);
                const float *k = in.kps + 5 * (uint64_t)in.obs_row[pos];
                c.x = k[0], c.y = k[1];
                cost = cost + rs_cost(cam_c[img], K, c, thr2);
            }
        }
        cost = combine(cost);
        if (alive && w.l == 0) {
            pt_c[3 * t] = c.X, pt_c[3 * t + 1] = c.Y, pt_c[3 * t + 2] = c.Z;
            sc.tcost[t] = cost;
        }
    }
}

// ---- the end ----------------------------------------------------------------------------------------------------------------------
// (kI: and the image's intrinsics, the f64 products rounded for an image of a free group, the input's words elsewhere; then a
// thread per group for d_group_out)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_final_images(SceneTables in, BaIntr gi, const float *poses, BaScratch sc, float *poses_out,
                                                            float *intrinsics_out, float *group_out) {
    const uint64_t img = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if constexpr (kI) {
        if (img >= in.n_images && img - in.n_images < gi.n_groups && group_out) {
            const uint64_t g = img - in.n_images;
            const BaGroup S = gi.gstate[(uint64_t)sc.words[kWCur] * gi.n_groups + g];
            group_out[3 * g] = float(S.s), group_out[3 * g + 1] = float(S.dx), group_out[3 * g + 2] = float(S.dy);
        }
        if (img < in.n_images) {
            const unsigned *ksrc = reinterpret_cast<const unsigned *>(in.intrinsics) + 4 * img;
            unsigned kw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) kw[i] = ksrc[i];
            const unsigned g = group_of(gi, (unsigned)img);
            if (group_free(gi, g)) {
                float K0[4], Kr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) K0[i] = __uint_as_float(kw[i]);
                ba_round_k(K0, gi.gstate[(uint64_t)sc.words[kWCur] * gi.n_groups + g], Kr);
#pragma unroll
                for (int i = 0; i < 4; ++i) kw[i] = __float_as_uint(Kr[i]);
            }
            unsigned *kdst = reinterpret_cast<unsigned *>(intrinsics_out) + 4 * img;
#pragma unroll
            for (int i = 0; i < 4; ++i) kdst[i] = kw[i];
        }
    }
    if (img >= in.n_images) return;
    const unsigned *src = reinterpret_cast<const unsigned *>(poses) + 12 * img;
    unsigned *dst = reinterpret_cast<unsigned *>(poses_out) + 12 * img;
    unsigned words[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) words[i] = src[i];
    if (sc.head[2 * img + 1] & kBaCamFree) {
        float P[12];
        ba_round_pose(sc.cam[(uint64_t)sc.words[kWCur] * in.n_images + img], P);
#pragma unroll
        for (int i = 0; i < 12; ++i) words[i] = __float_as_uint(P[i]);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = words[i];
}

// (kI: judged under intrinsics_out, and a fifth count)
template <bool kI>
__global__ __launch_bounds__(kThreads) void ba_final_tracks(SceneTables in, const float *points, double thr2, BaScratch sc,
                                                            const float *__restrict__ poses_out,
                                                            const float *__restrict__ intrinsics_out, float *points_out,
                                                            unsigned *obs_state_out, unsigned *__restrict__ counts_out) {
    const TrackWalk w = track_walk(in);
    const double *pt = sc.pt + (uint64_t)sc.words[kWCur] * in.tcap * 3;
    if (blockIdx.x == 0 && threadIdx.x < (kI ? 5 : 4)) {
        const int which = threadIdx.x == 0 ? kWFreeCams : threadIdx.x == 1 ? kWFreePoints : threadIdx.x == 2 ? kWActive
                          : threadIdx.x == 3 ? kWAccepted : kWFreeGroups;
        counts_out[threadIdx.x] = sc.words[which];
    }
    for (uint64_t t0 = w.first; t0 < w.T; t0 += w.stride) {                       // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < w.T;
        uint64_t lo = 0, hi = 0;
        unsigned words[4] = {0, 0, 0, 0};
        double X[3] = {0.0, 0.0, 0.0};
        if (alive) {
            track_range(in, t, w.O, lo, hi);
            const unsigned *src = reinterpret_cast<const unsigned *>(points) + 4 * t;
#pragma unroll
            for (int k = 0; k < 4; ++k) words[k] = src[k];
            if (sc.tflag[t] & kBaPointFree) {
#pragma unroll
                for (int k = 0; k < 3; ++k) words[k] = __float_as_uint(float(pt[3 * t + k]));
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) X[k] = double(__uint_as_float(words[k]));
        }
        const unsigned nch = obs_state_out ? (unsigned)((hi - lo + G - 1) / G) : 0u;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            const uint64_t pos = lo + (uint64_t)ch * G + w.l;
            if (ch < nch && pos < hi) {
                unsigned state = 0;
                if (sc.oflag[pos] & kBaActive) {
                    const unsigned img = in.obs_image[pos];
                    const float *k = in.kps + 5 * (uint64_t)in.obs_row[pos];
                    TriObs o;
                    o.x = k[0], o.y = k[1];
#pragma unroll
                    for (int i = 0; i < 4; ++i) o.K[i] = (kI ? intrinsics_out : in.intrinsics)[4 * (uint64_t)img + i];
#pragma unroll
                    for (int i = 0; i < 12; ++i) o.P[i] = poses_out[12 * (uint64_t)img + i];
                    double e2;
                    state = tri_inlier(o, X, thr2, e2) ? 2u : 1u;
                }
                obs_state_out[pos] = state;
            }
        }
        if (alive && w.l == 0) {
            unsigned *dst = reinterpret_cast<unsigned *>(points_out) + 4 * t;
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k] = words[k];
        }
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
namespace {
struct BaLayout {
    uint64_t cam, pt, U, V, W, vec, y, tcost, dots, scal, rowmap, idx, head, oflag, tflag, words;
    uint64_t gstate, gU, gvec, gdots, Uck, ipart, icount, gflag, total;      // the intrinsics call's own, behind the rest
};
BaLayout layout(uint64_t n_images, uint64_t n_rows, uint64_t tcap, uint64_t ocap, bool intrinsics, uint64_t n_groups) {
    BaLayout L;
    uint64_t at = 0;
    const auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at += (bytes + 15) / 16 * 16;
        return here;
    };
    L.cam = take(8 * 2 * 12 * n_images);
    L.pt = take(8 * 2 * 3 * tcap);
    L.U = take(8 * kRsTerms * n_images);
    L.V = take(8 * kBaPointTerms * tcap);
#ifdef LF_BA_STORE_W
    L.W = take(8 * kBaW * ocap);
#else
    L.W = take(0);
#endif
    L.vec = take(8 * kVecs * 6 * n_images);
    L.y = take(8 * 3 * tcap);
    L.tcost = take(8 * tcap);
    L.dots = take(8 * n_images);
    L.scal = take(8 * kScalars);
    L.rowmap = take(8 * n_rows);
    L.idx = take(4 * n_rows);
    L.head = take(4 * 2 * n_images);
    L.oflag = take(4 * ocap);
    L.tflag = take(4 * tcap);
    L.words = take(4 * kWords);
    L.gstate = L.gU = L.gvec = L.gdots = L.Uck = L.ipart = L.icount = L.gflag = at;
    if (intrinsics) {
        L.gstate = take(8 * 2 * 3 * n_groups);
        L.gU = take(8 * kBaGroupTerms * n_groups);
        L.gvec = take(8 * kVecs * 3 * n_groups);
        L.gdots = take(8 * n_groups);
        L.Uck = take(8 * kBaCk * n_images);
        L.ipart = take(8 * 12 * n_images);
        L.icount = take(4 * n_images);
        L.gflag = take(4 * n_groups);
    }
    L.total = at;
    return L;
}

// The one launch sequence of both calls: kI = false is lf_mkd_bundle_adjust_device's, kI = true adds ba_setup_groups, a
// ba_group_lin per iteration and a ba_group_apply per CG step, and the thread-per-image kernels take n_groups more threads.
template <bool kI>
void launch(void *scratch, const SceneTables &in, const unsigned *group, unsigned n_groups, unsigned refine, const float *points,
            const float *poses, const unsigned *obs_state, const unsigned *camera_fixed, double thr2, double lambda0, unsigned iterations,
            unsigned cg_iterations, double tol2, float *poses_out, float *points_out, float *intrinsics_out, float *group_out,
            unsigned *obs_state_out, double *trace, unsigned *counts, hipStream_t stream) {
    const unsigned n_images = in.n_images;
    const uint64_t n_rows = in.n_rows, track_capacity = in.tcap;
    unsigned char *b = static_cast<unsigned char *>(scratch);
    const BaLayout L = layout(n_images, n_rows, track_capacity, in.ocap, kI, n_groups);
    const auto f64 = [&](uint64_t at) { return reinterpret_cast<double *>(b + at); };
    const auto u32 = [&](uint64_t at) { return reinterpret_cast<unsigned *>(b + at); };
    const BaScratch sc = {reinterpret_cast<RsPose *>(b + L.cam), f64(L.pt), f64(L.U), f64(L.V), f64(L.W), f64(L.vec), f64(L.y),
                          f64(L.tcost), f64(L.dots), f64(L.scal), reinterpret_cast<unsigned long long *>(b + L.rowmap), u32(L.idx),
                          u32(L.head), u32(L.oflag), u32(L.tflag), u32(L.words)};
    const BaIntr gi = {group, n_groups, refine, reinterpret_cast<BaGroup *>(b + L.gstate), f64(L.gU), f64(L.gvec), f64(L.gdots),
                       f64(L.Uck), f64(L.ipart), u32(L.icount), u32(L.gflag)};
    const auto blocks = [](uint64_t items, uint64_t per_block) {
        const uint64_t want = (items + per_block - 1) / per_block;
        return dim3((unsigned)(want < 1 ? 1 : want < kMaxBlocks ? want : kMaxBlocks));
    };
    const uint64_t singles = (uint64_t)n_images + (kI ? n_groups : 0u);             // a thread per image, then one per group
    const dim3 threads(kThreads), per_image(n_images), by_image((unsigned)((singles + kThreads - 1) / kThreads)), per_group(n_groups);
    const dim3 by_track = blocks(track_capacity, kThreads / G);
    uint64_t most = n_rows > n_images ? n_rows : n_images;
    if (kI && n_groups > most) most = n_groups;
    hipLaunchKernelGGL(ba_init<kI>, blocks(most > 16 ? most : 16, kThreads), threads, 0, stream, in, gi, poses, camera_fixed, lambda0, sc);
    hipLaunchKernelGGL(ba_setup_tracks, by_track, threads, 0, stream, in, points, obs_state, sc);
    hipLaunchKernelGGL(ba_setup_images<kI>, per_image, threads, 0, stream, in, sc);
    if constexpr (kI) hipLaunchKernelGGL(ba_setup_groups, per_group, threads, 0, stream, in, gi, sc);
    for (unsigned it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(ba_track_lin<kI>, by_track, threads, 0, stream, in, gi, thr2, sc);
        hipLaunchKernelGGL(ba_image_lin<kI>, per_image, threads, 0, stream, in, gi, thr2, sc);
        if constexpr (kI) hipLaunchKernelGGL(ba_group_lin, per_group, threads, 0, stream, in, gi, sc);
        hipLaunchKernelGGL(ba_scalar<kI>, dim3(1), threads, 0, stream, in, gi, (unsigned)kModeStart, tol2, it, sc, trace);
        for (unsigned s = 0; s < cg_iterations; ++s) {
            hipLaunchKernelGGL(ba_track_apply<kI>, by_track, threads, 0, stream, in, gi, sc);
            hipLaunchKernelGGL(ba_image_apply<kI>, per_image, threads, 0, stream, in, gi, sc);
            if constexpr (kI) hipLaunchKernelGGL(ba_group_apply, per_group, threads, 0, stream, in, gi, sc);
            hipLaunchKernelGGL(ba_scalar<kI>, dim3(1), threads, 0, stream, in, gi, (unsigned)kModeAlpha, tol2, it, sc, trace);
            hipLaunchKernelGGL(ba_cg_update<kI>, by_image, threads, 0, stream, in, gi, sc);
            hipLaunchKernelGGL(ba_scalar<kI>, dim3(1), threads, 0, stream, in, gi, (unsigned)kModeBeta, tol2, it, sc, trace);
        }
        hipLaunchKernelGGL(ba_cam_step<kI>, by_image, threads, 0, stream, in, gi, sc);
        hipLaunchKernelGGL(ba_track_step<kI>, by_track, threads, 0, stream, in, gi, thr2, sc);
        hipLaunchKernelGGL(ba_scalar<kI>, dim3(1), threads, 0, stream, in, gi, (unsigned)kModeAccept, tol2, it, sc, trace);
    }
    hipLaunchKernelGGL(ba_final_images<kI>, by_image, threads, 0, stream, in, gi, poses, sc, poses_out, intrinsics_out, group_out);
    hipLaunchKernelGGL(ba_final_tracks<kI>, by_track, threads, 0, stream, in, points, thr2, sc, poses_out, intrinsics_out, points_out,
                       obs_state_out, counts);
}
}  // namespace

uint64_t bundle_scratch_bytes(unsigned n_images, uint64_t n_rows, uint64_t track_capacity, uint64_t obs_capacity) {
    return layout(n_images, n_rows, track_capacity, obs_capacity, false, 0).total;
}
unsigned bundle_launches(unsigned iterations, unsigned cg_iterations) { return 5 + iterations * (6 + 5 * cg_iterations); }

void launch_bundle_adjust(void *scratch, const SceneTables &in, const float *points, const float *poses, const unsigned *obs_state,
                          const unsigned *camera_fixed, double thr2, double lambda0, unsigned iterations, unsigned cg_iterations,
                          double tol2, float *poses_out, float *points_out, unsigned *obs_state_out, double *trace, unsigned *counts,
                          hipStream_t stream) {
    if (in.n_images == 0) return;
    launch<false>(scratch, in, nullptr, 0, 0, points, poses, obs_state, camera_fixed, thr2, lambda0, iterations, cg_iterations, tol2,
                  poses_out, points_out, nullptr, nullptr, obs_state_out, trace, counts, stream);
}

uint64_t bundle_intrinsics_scratch_bytes(unsigned n_images, uint64_t n_rows, uint64_t track_capacity, uint64_t obs_capacity,
                                         unsigned n_groups) {
    return layout(n_images, n_rows, track_capacity, obs_capacity, true, n_groups).total;
}
unsigned bundle_intrinsics_launches(unsigned iterations, unsigned cg_iterations) { return 6 + iterations * (7 + 6 * cg_iterations); }

void launch_bundle_adjust_intrinsics(void *scratch, const SceneTables &in, const float *points, const float *poses,
                                     const unsigned *obs_state, const unsigned *camera_fixed, const unsigned *camera_group,
                                     unsigned n_groups, unsigned refine, double thr2, double lambda0, unsigned iterations,
                                     unsigned cg_iterations, double tol2, float *poses_out, float *points_out, float *intrinsics_out,
                                     float *group_out, unsigned *obs_state_out, double *trace, unsigned *counts, hipStream_t stream) {
    if (in.n_images == 0) return;
    launch<true>(scratch, in, camera_group, n_groups, refine, points, poses, obs_state, camera_fixed, thr2, lambda0, iterations,
                 cg_iterations, tol2, poses_out, points_out, intrinsics_out, group_out, obs_state_out, trace, counts, stream);
}

}  // namespace lfmkd
