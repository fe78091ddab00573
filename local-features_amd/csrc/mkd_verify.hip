// gfx950 RANSAC verification of matches: homography (lf_mkd_verify_homography*) and fundamental matrix
// (lf_mkd_verify_fundamental*, include/lf_mkd.h).  One kernel pair, ransac_score<Model> / ransac_select<Model>, instantiated
// with HomographyModel (mkd_homography_math.h) and FundamentalModel (mkd_fundamental_math.h).
//
// Three launches per call, whatever the number of pairs, none of which waits on another workgroup:
//
//   verify_prepare  one workgroup per pair: lists the pair's considered matches (0 <= match[i] < nb) by ascending i --
//                   the list is written into the caller's `verified` rows of that pair, which the last launch overwrites --
//                   and the per-pair normalisation (centroid, RMS distance sqrt(2)) of both point sets, into VerifyPair.
//   ransac_score    the hot path.  One lane per sample: it draws its matches (counter-based sampler) and solves the minimal
//                   problem in registers -- H: 4 matches, square -> quad twice, H = B adj(A), one candidate; F: 7 matches,
//                   the 7 x 9 system's null space by Gauss-Jordan elimination with full pivoting, the real roots of
//                   det(l F1 + (1 - l) F2) = 0 bracketed and polished, up to three candidates (27 floats) -- then walks the
//                   pair's rows, whose considered points the workgroup stages through LDS as float4 {ax, ay, bx, by} 256
//                   rows at a time; every lane reads the same LDS address (a broadcast) and keeps its counts in registers.
//                   Grid = (pair, block of 256 samples, row slice): the slices (at most 16) split a pair's rows so that a
//                   call with few pairs still spreads over up to ~2 x CUs workgroups; each writes its partial counts
//                   [pair][slice][sample][kCand].
//   ransac_select   one workgroup per pair: argmax of the summed counts on the key (count, -c), c = kCand k + j, by wave
//                   reductions, the winner recomputed by the same code, the least-squares refit (normal equations in f64,
//                   8x8 Cholesky in registers -- H: 23 moments, h8 = 1; F: 36 moments, the largest entry pinned to 1, rank
//                   2 by a cyclic Jacobi of F^T F; a refit is kept if its truncated quadratic (MSAC) cost does not rise),
//                   the final rescoring, and the model, verified, stats.
//
// What determines the bits: every step is a fixed sequence of IEEE operations -- this file and the math headers are
// compiled with contraction OFF (the pragma below) and state their fused operations as fmaf; F's root finder uses only
// correctly rounded operations (+ - * /, sqrtf, fmaf) with fixed iteration counts -- so a sample's candidates and every
// point's inlier test give the same bits in ransac_score and ransac_select, for any slicing of the rows, any number of
// pairs in the call, and any run.  Sums (normalisation f32, refit f64) run in a fixed per-thread order and a fixed tree.
// The math headers are __host__ __device__: a host build of them gives the same bits.  tests/cpp/fundamental_twin.cpp is
// that build for F (g++ with -ffp-contract=off, restating only these kernels' orchestration):
// tests/test_gpu_fundamental_exact.py holds the device to it bit for bit, sample by sample, and
// tests/test_fundamental_twin.py holds it to the float64 restatement of include/lf_mkd.h on the CPU.  H is held to the numpy
// f32 twin tests/homography_f32.py (tests/test_gpu_homography_exact.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mkd_fundamental_math.h"
#include "mkd_homography_math.h"
#include "mkd_verify_common.h"

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

// ---- launch 1: considered matches + normalisation ---------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void verify_prepare(const float *kps_a, const uint64_t *off_a, const float *kps_b,
                                                           const uint64_t *off_b, const int *match, int *list,
                                                           VerifyPair *pairs) {
    __shared__ unsigned wtot[kWaves];
    __shared__ float red[kWaves * 4];
    const unsigned p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t oa, ob;
    const uint64_t na = pair_rows(off_a, p, oa), nb = pair_rows(off_b, p, ob);
    const float *ka = kps_a + 5 * oa, *kb = kps_b + 5 * ob;
    const int *mt = match + oa;
    int *ls = list + oa;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned base = 0;
    for (uint64_t r0 = 0; r0 < na; r0 += kThreads) {
        const uint64_t r = r0 + tid;
        Pt q;
        const bool c = r < na && load_row(ka, kb, mt, r, nb, q);
        if (c) {
            s[0] += q.ax;
            s[1] += q.ay;
            s[2] += q.bx;
            s[3] += q.by;
        }
        const unsigned long long bal = __ballot(c);
        const unsigned before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = unsigned(__popcll(bal));
        __syncthreads();
        unsigned at = base, tot = 0;
        for (int w = 0; w < kWaves; ++w) {
            at += w < wave ? wtot[w] : 0u;
            tot += wtot[w];
        }
        if (c) ls[at + before] = int(r);
        base += tot;
        __syncthreads();
    }
    block_sum<float, 4>(s, red);
    const unsigned M = base;
    const float inv = M ? 1.f / float(M) : 0.f;
    const float cax = s[0] * inv, cay = s[1] * inv, cbx = s[2] * inv, cby = s[3] * inv;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint64_t r = tid; r < na; r += kThreads) {
        Pt q;
        if (!load_row(ka, kb, mt, r, nb, q)) continue;
        const float x = q.ax - cax, y = q.ay - cay, u = q.bx - cbx, v = q.by - cby;
        d[0] += x * x + y * y;
        d[1] += u * u + v * v;
    }
    block_sum<float, 4>(d, red);
    if (tid == 0) {
        VerifyPair P;
        P.ca[0] = cax;
        P.ca[1] = cay;
        P.cb[0] = cbx;
        P.cb[1] = cby;
        P.sa = d[0] > 0.f ? sqrtf(2.f * float(M) / d[0]) : 1.f;
        P.sb = d[1] > 0.f ? sqrtf(2.f * float(M) / d[1]) : 1.f;
        P.m = M;
        P.pad = 0;
        pairs[p] = P;
    }
}


// A Model (HomographyModel, FundamentalModel) is a struct of compile-time constants and static functions:
//   kCand, kMoments, kRows   candidates per sample; f64 moments of the refit; rows per unrolled step of the scoring loop
//   candidates(...)          sample k of a pair -> its candidates' valid bits, pixel forms f and normalised forms fn
//   inlier, inlier_cost      one point's test under a pixel model, and its share of the cost the refit is judged by
//   add_moments              one inlier's (normalised) share of the refit's moments
//   refit(m, fn, P, fn2, f2) the summed moments and the current normalised model -> the refitted model; false if it fails
//   pivot(f)                 the entry the output model is divided by
// ---- launch 2: one lane per sample, counts of its candidates over a slice of the pair's rows --------------------------
template <class Model>
__global__ __launch_bounds__(kThreads) void ransac_score(const float *kps_a, const uint64_t *off_a, const float *kps_b,
                                                         const uint64_t *off_b, const int *match, const int *list,
                                                         const VerifyPair *pairs, unsigned n_hyp, unsigned hyp_blocks,
                                                         unsigned slices, float thr2, unsigned seed, unsigned *counts) {
    constexpr int kCand = Model::kCand;
    __shared__ f32x4 tile[kThreads];
    __shared__ unsigned wtot[kWaves];
    const unsigned id = blockIdx.x;
    const unsigned sl = id % slices, hb = (id / slices) % hyp_blocks, p = id / slices / hyp_blocks;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t oa, ob;
    const uint64_t na = pair_rows(off_a, p, oa), nb = pair_rows(off_b, p, ob);
    const float *ka = kps_a + 5 * oa, *kb = kps_b + 5 * ob;
    const int *mt = match + oa;
    const VerifyPair P = pairs[p];
    const unsigned k = hb * kThreads + tid;
    float f[kCand][9], fn[kCand][9];
    const unsigned valid = k < n_hyp ? Model::candidates(ka, kb, mt, list + oa, P, seed + p, k, f, fn) : 0u;
    unsigned cnt[kCand] = {};
    if (__syncthreads_or(valid != 0u)) {
        const uint64_t lo = na * sl / slices, hi = na * (sl + 1) / slices;
        for (uint64_t r0 = lo; r0 < hi; r0 += kThreads) {
            const uint64_t r = r0 + tid;
            Pt q;
            const bool c = r < hi && load_row(ka, kb, mt, r, nb, q);
            const unsigned long long bal = __ballot(c);
            if (lane == 0) wtot[wave] = unsigned(__popcll(bal));
            __syncthreads();
            unsigned at = __popcll(bal & ((1ull << lane) - 1ull)), n = 0;
            for (int w = 0; w < kWaves; ++w) {
                at += w < wave ? wtot[w] : 0u;
                n += wtot[w];
            }
            if (c) tile[at] = f32x4{q.ax, q.ay, q.bx, q.by};
            __syncthreads();
            if (valid) {
                const auto row = [&](unsigned j) {
                    const f32x4 t = tile[j];
#pragma unroll
                    for (int u = 0; u < kCand; ++u) cnt[u] += Model::inlier(f[u], t.x, t.y, t.z, t.w, thr2);
                };
                unsigned j = 0;
                if constexpr (Model::kRows > 1)
                    for (; j + Model::kRows <= n; j += Model::kRows)
#pragma unroll
                        for (int u = 0; u < Model::kRows; ++u) row(j + u);
                for (; j < n; ++j) row(j);
            }
            __syncthreads();
        }
    }
    if (k < n_hyp) {
        unsigned *out = counts + ((uint64_t(p) * slices + sl) * n_hyp + k) * kCand;
#pragma unroll
        for (int u = 0; u < kCand; ++u) out[u] = (valid >> u) & 1u ? cnt[u] : kInvalid;
    }
}

// ---- launch 3: selection, refit, outputs ------------------------------------------------------------------------------
template <class Model>
__global__ __launch_bounds__(kThreads) void ransac_select(const float *kps_a, const uint64_t *off_a, const float *kps_b,
                                                          const uint64_t *off_b, const int *match, int *verified,
                                                          const VerifyPair *pairs, const unsigned *counts, unsigned n_hyp,
                                                          unsigned slices, float thr2, unsigned seed, unsigned flags,
                                                          float *model_out, unsigned *stats) {
    constexpr int kCand = Model::kCand, kMoments = Model::kMoments;
    __shared__ unsigned long long kred[kWaves];
    __shared__ double dred[kWaves * kMoments];
    __shared__ unsigned ured[kWaves * 2];
    const unsigned p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t oa, ob;
    const uint64_t na = pair_rows(off_a, p, oa), nb = pair_rows(off_b, p, ob);
    const float *ka = kps_a + 5 * oa, *kb = kps_b + 5 * ob;
    const int *mt = match + oa;
    int *ver = verified + oa;
    const VerifyPair P = pairs[p];
    // argmax on (count, -c) over the candidates c = kCand k + j; an invalid one has key 0
    unsigned long long best = 0;
    const unsigned n_cand = kCand * n_hyp;
    const unsigned *cp = counts + uint64_t(p) * slices * n_cand;
    for (unsigned c = tid; c < n_cand; c += kThreads) {
        const unsigned c0 = cp[c];
        if (c0 == kInvalid) continue;
        // the slices' partial counts, 8 loads in flight at a time (a chain of single loads made this launch the call's cost)
        unsigned t = c0, s = 1;
        for (; s + 8 <= slices; s += 8) {
            unsigned v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = cp[uint64_t(s + j) * n_cand + c];
#pragma unroll
            for (int j = 0; j < 8; ++j) t += v[j];
        }
        for (; s < slices; ++s) t += cp[uint64_t(s) * n_cand + c];
        best = max(best, ((unsigned long long)(t + 1u) << 32) | (unsigned long long)(kInvalid - c));
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, o));
    if (lane == 0) kred[wave] = best;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) best = max(best, kred[w]);
    const bool found = best != 0;
    const unsigned c_best = found ? kInvalid - unsigned(best & 0xFFFFFFFFull) : kInvalid;
    const unsigned best_count = found ? unsigned(best >> 32) - 1u : 0u;
    // every thread recomputes the winner: the same bits as in ransac_score
    float f[9], fn[9];
    bool have = false;
    {
        float fa[kCand][9], fna[kCand][9];
        const unsigned k_best = found ? c_best / kCand : 0u, j_best = found ? c_best % kCand : 0u;
        const unsigned ok = found ? Model::candidates(ka, kb, mt, verified + oa, P, seed + p, k_best, fa, fna) : 0u;
        have = (ok >> j_best) & 1u;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            f[i] = fa[0][i];
            fn[i] = fna[0][i];
#pragma unroll
            for (int j = 1; j < kCand; ++j) {
                f[i] = j_best == unsigned(j) ? fa[j][i] : f[i];
                fn[i] = j_best == unsigned(j) ? fna[j][i] : fn[i];
            }
        }
    }
    __syncthreads();   // the list of considered rows in `verified` has been read: from here on it is output
    unsigned final_count = 0;
    if (have) {
        const bool refine = !(flags & 1u);
        double m[kMoments];
        unsigned n_cur = 0;
        double cost_cur = 0.0;
#pragma unroll
        for (int i = 0; i < kMoments; ++i) m[i] = 0.0;
        for (uint64_t r = tid; r < na; r += kThreads) {
            Pt q;
            float e;
            if (!load_row(ka, kb, mt, r, nb, q)) continue;
            const bool in = Model::inlier_cost(f, q.ax, q.ay, q.bx, q.by, thr2, e);
            cost_cur += e;
            if (!in) continue;
            ++n_cur;
            if (refine)
                Model::add_moments(m, double((q.ax - P.ca[0]) * P.sa), double((q.ay - P.ca[1]) * P.sa),
                                   double((q.bx - P.cb[0]) * P.sb), double((q.by - P.cb[1]) * P.sb));
        }
        {
            unsigned v[1] = {n_cur};
            block_sum<unsigned, 1>(v, ured);
            n_cur = v[0];
            double cc[1] = {cost_cur};
            block_sum<double, 1>(cc, dred);
            cost_cur = cc[0];
        }
        for (int round = 0; refine && round < 3; ++round) {
            block_sum<double, kMoments>(m, dred);
            float fn2[9], f2[9];
            if (!Model::refit(m, fn, P, fn2, f2)) break;
#pragma unroll
            for (int i = 0; i < kMoments; ++i) m[i] = 0.0;   // (from here on: the refit's own moments; no exit reads m again)
            unsigned c[2] = {0u, 0u};   // inliers of the refit, points whose membership changed
            double cost[1] = {0.0};     // the refit's truncated quadratic (MSAC) cost
            for (uint64_t r = tid; r < na; r += kThreads) {
                Pt q;
                float e;
                if (!load_row(ka, kb, mt, r, nb, q)) continue;
                const bool in_old = Model::inlier(f, q.ax, q.ay, q.bx, q.by, thr2);
                const bool in_new = Model::inlier_cost(f2, q.ax, q.ay, q.bx, q.by, thr2, e);
                cost[0] += e;
                c[1] += in_old != in_new;
                if (!in_new) continue;
                ++c[0];
                Model::add_moments(m, double((q.ax - P.ca[0]) * P.sa), double((q.ay - P.ca[1]) * P.sa),
                                   double((q.bx - P.cb[0]) * P.sb), double((q.by - P.cb[1]) * P.sb));
            }
            block_sum<unsigned, 2>(c, ured);
            block_sum<double, 1>(cost, dred);
            if (cost[0] > cost_cur) break;   // a refit whose cost rises is not kept
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                f[i] = f2[i];
                fn[i] = fn2[i];
            }
            n_cur = c[0];
            cost_cur = cost[0];
            if (c[1] == 0) break;      // the inlier set stopped changing
        }
        final_count = n_cur;
    }
    // outputs: verified (every row of the pair), the model divided by its pivot (H[8]; F's entry of largest magnitude), stats
    for (uint64_t r = tid; r < na; r += kThreads) {
        Pt q;
        const int mm = mt[r];
        ver[r] = have && load_row(ka, kb, mt, r, nb, q) && Model::inlier(f, q.ax, q.ay, q.bx, q.by, thr2) ? mm : -1;
    }
    if (tid < 9) model_out[9 * uint64_t(p) + tid] = have ? f[tid] / Model::pivot(f) : 0.f;
    if (tid < 4) {
        const unsigned st[4] = {have ? final_count : 0u, have ? best_count : 0u, have ? c_best : kInvalid, P.m};
        stats[4 * uint64_t(p) + tid] = tid == 0 ? st[0] : tid == 1 ? st[1] : tid == 2 ? st[2] : st[3];
    }
}

template <class Model>
void launch_ransac(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                   unsigned n_pairs, unsigned n_hyp, float threshold, unsigned seed, unsigned flags, unsigned slices,
                   VerifyPair *pairs, unsigned *counts, float *model, int *verified, unsigned *stats, hipStream_t stream) {
    if (n_pairs == 0) return;
    const float thr2 = threshold * threshold;
    const unsigned hyp_blocks = (n_hyp + kThreads - 1) / kThreads;
    launch_verify_prepare(kps_a, off_a, kps_b, off_b, match, n_pairs, pairs, verified, stream);
    hipLaunchKernelGGL(ransac_score<Model>, dim3(n_pairs * hyp_blocks * slices), dim3(kThreads), 0, stream, kps_a, off_a,
                       kps_b, off_b, match, verified, pairs, n_hyp, hyp_blocks, slices, thr2, seed, counts);
    hipLaunchKernelGGL(ransac_select<Model>, dim3(n_pairs), dim3(kThreads), 0, stream, kps_a, off_a, kps_b, off_b, match,
                       verified, pairs, counts, n_hyp, slices, thr2, seed, flags, model, stats);
}

}  // namespace

unsigned verify_slices(unsigned n_pairs, unsigned n_hyp, int num_cus) {
    const uint64_t blocks = uint64_t(n_pairs) * ((n_hyp + kThreads - 1) / kThreads);
    const uint64_t want = (uint64_t(2 * num_cus) + blocks - 1) / blocks;
    return unsigned(want < 1 ? 1 : want > kMaxSlices ? kMaxSlices : want);
}

void launch_verify_prepare(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                           unsigned n_pairs, VerifyPair *pairs, int *list, hipStream_t stream) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(verify_prepare, dim3(n_pairs), dim3(kThreads), 0, stream, kps_a, off_a, kps_b, off_b, match, list, pairs);
}

void launch_verify(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                   unsigned n_pairs, unsigned n_hyp, float threshold, unsigned seed, unsigned flags, unsigned slices,
                   VerifyPair *pairs, unsigned *counts, float *H, int *verified, unsigned *stats, hipStream_t stream) {
    launch_ransac<HomographyModel>(kps_a, off_a, kps_b, off_b, match, n_pairs, n_hyp, threshold, seed, flags, slices, pairs,
                                   counts, H, verified, stats, stream);
}

void launch_fundamental(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                        unsigned n_pairs, unsigned n_hyp, float threshold, unsigned seed, unsigned flags, unsigned slices,
                        VerifyPair *pairs, unsigned *counts, float *F, int *verified, unsigned *stats, hipStream_t stream) {
    launch_ransac<FundamentalModel>(kps_a, off_a, kps_b, off_b, match, n_pairs, n_hyp, threshold, seed, flags, slices, pairs,
                                    counts, F, verified, stats, stream);
}

}  // namespace lfmkd
