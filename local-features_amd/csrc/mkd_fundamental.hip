// gfx950 RANSAC fundamental-matrix verification of matches (lf_mkd_verify_fundamental*, include/lf_mkd.h).
//
// Three launches per call, whatever the number of pairs, none of which waits on another workgroup:
//
//   verify_prepare      mkd_verify.hip's first launch, as it is (launch_verify_prepare): each pair's considered rows into
//                       the caller's `verified` rows, and the pair's normalisation.
//   fundamental_score   the hot path.  One lane per sample: it draws 7 matches (counter-based sampler), finds the 7 x 9
//                       system's null space by Gauss-Jordan elimination with full pivoting, brackets and polishes the real
//                       roots of det(l F1 + (1 - l) F2) = 0, and holds up to three candidates (27 floats) and their counts in
//                       registers; then it walks the pair's rows, which the workgroup stages through LDS as float4
//                       {ax, ay, bx, by} 256 rows at a time (every lane reads the same address: a broadcast), testing each
//                       against the three candidates' Sampson distance.  Grid = (pair, block of 256 samples, row slice), as
//                       verify_score's; each workgroup writes its partial counts [pair][slice][sample][3].
//   fundamental_select  one workgroup per pair: argmax of the summed counts on the key (count, -c), c = 3 k + j, the winner
//                       recomputed by the same code, the least-squares refit (36 f64 moments, 8x8 Cholesky with the largest
//                       entry pinned to 1, rank 2 by a cyclic Jacobi of F^T F; kept if the MSAC cost does not rise), the
//                       final rescoring, and F, verified, stats.
//
// What determines the bits: as in mkd_verify.hip, every step is a fixed sequence of IEEE operations (contraction OFF, fused
// operations written as fmaf), and the root finder uses only correctly rounded operations (+ - * /, sqrtf, fmaf) with fixed
// iteration counts, so a sample's candidates and every point's test give the same bits in both launches and any slicing.
// The math helpers (mkd_fundamental_math.h) are __host__ __device__: a host build of them gives the same bits (fmaf and sqrtf
// are correctly rounded).  That build exists -- tests/cpp/fundamental_twin.cpp, g++ with -ffp-contract=off, restating only these
// kernels' orchestration -- and tests/test_gpu_fundamental_exact.py holds the device to it bit for bit, sample by sample;
// tests/test_fundamental_twin.py holds it to the float64 restatement of include/lf_mkd.h on the CPU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mkd_fundamental_math.h"
#include "mkd_verify_common.h"

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

// ---- launch 2: one lane per sample, counts of its three candidates over a slice of the pair's rows -------------------
__global__ __launch_bounds__(kThreads) void fundamental_score(const float *kps_a, const uint64_t *off_a, const float *kps_b,
                                                              const uint64_t *off_b, const int *match, const int *list,
                                                              const VerifyPair *pairs, unsigned n_hyp, unsigned hyp_blocks,
                                                              unsigned slices, float thr2, unsigned seed, unsigned *counts) {
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
    float f[3][9], fn[3][9];
    const unsigned valid = k < n_hyp ? candidates(ka, kb, mt, list + oa, P, seed + p, k, f, fn) : 0u;
    unsigned cnt[3] = {0u, 0u, 0u};
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
                for (unsigned j = 0; j < n; ++j) {
                    const f32x4 t = tile[j];
#pragma unroll
                    for (int u = 0; u < 3; ++u) cnt[u] += f_inlier(f[u], t.x, t.y, t.z, t.w, thr2);
                }
            }
            __syncthreads();
        }
    }
    if (k < n_hyp) {
        unsigned *out = counts + ((uint64_t(p) * slices + sl) * n_hyp + k) * 3;
#pragma unroll
        for (int u = 0; u < 3; ++u) out[u] = (valid >> u) & 1u ? cnt[u] : kInvalid;
    }
}

// ---- launch 3: selection, refit, outputs ------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fundamental_select(const float *kps_a, const uint64_t *off_a, const float *kps_b,
                                                               const uint64_t *off_b, const int *match, int *verified,
                                                               const VerifyPair *pairs, const unsigned *counts, unsigned n_hyp,
                                                               unsigned slices, float thr2, unsigned seed, unsigned flags,
                                                               float *F_out, unsigned *stats) {
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
    // argmax on (count, -c) over the candidates c = 3 k + j; an invalid one has key 0
    unsigned long long best = 0;
    const unsigned n_cand = 3 * n_hyp;
    const unsigned *cp = counts + uint64_t(p) * slices * n_cand;
    for (unsigned c = tid; c < n_cand; c += kThreads) {
        const unsigned c0 = cp[c];
        if (c0 == kInvalid) continue;
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
    // every thread recomputes the winner: the same bits as in fundamental_score
    float f[9], fn[9];
    bool have = false;
    {
        float fa[3][9], fna[3][9];
        const unsigned k_best = found ? c_best / 3u : 0u, j_best = found ? c_best % 3u : 0u;
        const unsigned ok = found ? candidates(ka, kb, mt, verified + oa, P, seed + p, k_best, fa, fna) : 0u;
        have = (ok >> j_best) & 1u;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            f[i] = j_best == 0 ? fa[0][i] : j_best == 1 ? fa[1][i] : fa[2][i];
            fn[i] = j_best == 0 ? fna[0][i] : j_best == 1 ? fna[1][i] : fna[2][i];
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
            const bool in = f_inlier_cost(f, q.ax, q.ay, q.bx, q.by, thr2, e);
            cost_cur += e;
            if (!in) continue;
            ++n_cur;
            if (refine)
                add_moments36(m, double((q.ax - P.ca[0]) * P.sa), double((q.ay - P.ca[1]) * P.sa),
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
            if (!refit_solve(m, argmax_abs9(fn), fn2) || !f_denormalise(fn2, P, f2)) break;
#pragma unroll
            for (int i = 0; i < kMoments; ++i) m[i] = 0.0;   // (from here on: the refit's own moments)
            unsigned c[2] = {0u, 0u};   // inliers of the refit, points whose membership changed
            double cost[1] = {0.0};     // the refit's MSAC cost
            for (uint64_t r = tid; r < na; r += kThreads) {
                Pt q;
                float e;
                if (!load_row(ka, kb, mt, r, nb, q)) continue;
                const bool in_old = f_inlier(f, q.ax, q.ay, q.bx, q.by, thr2);
                const bool in_new = f_inlier_cost(f2, q.ax, q.ay, q.bx, q.by, thr2, e);
                cost[0] += e;
                c[1] += in_old != in_new;
                if (!in_new) continue;
                ++c[0];
                add_moments36(m, double((q.ax - P.ca[0]) * P.sa), double((q.ay - P.ca[1]) * P.sa),
                              double((q.bx - P.cb[0]) * P.sb), double((q.by - P.cb[1]) * P.sb));
            }
            block_sum<unsigned, 2>(c, ured);
            block_sum<double, 1>(cost, dred);
            if (cost[0] > cost_cur) break;   // a refit whose MSAC cost rises is not kept
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
    // outputs: verified (every row of the pair), F divided by its entry of largest magnitude, stats
    for (uint64_t r = tid; r < na; r += kThreads) {
        Pt q;
        const int mm = mt[r];
        ver[r] = have && load_row(ka, kb, mt, r, nb, q) && f_inlier(f, q.ax, q.ay, q.bx, q.by, thr2) ? mm : -1;
    }
    if (tid < 9) {
        const int c = argmax_abs9(f);
        float piv = f[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) piv = i == c ? f[i] : piv;
        F_out[9 * uint64_t(p) + tid] = have ? f[tid] / piv : 0.f;
    }
    if (tid < 4) {
        const unsigned st[4] = {have ? final_count : 0u, have ? best_count : 0u, have ? c_best : kInvalid, P.m};
        stats[4 * uint64_t(p) + tid] = tid == 0 ? st[0] : tid == 1 ? st[1] : tid == 2 ? st[2] : st[3];
    }
}

}  // namespace

void launch_fundamental(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                        unsigned n_pairs, unsigned n_hyp, float threshold, unsigned seed, unsigned flags, unsigned slices,
                        VerifyPair *pairs, unsigned *counts, float *F, int *verified, unsigned *stats, hipStream_t stream) {
    if (n_pairs == 0) return;
    const float thr2 = threshold * threshold;
    const unsigned hyp_blocks = (n_hyp + kThreads - 1) / kThreads;
    launch_verify_prepare(kps_a, off_a, kps_b, off_b, match, n_pairs, pairs, verified, stream);
    hipLaunchKernelGGL(fundamental_score, dim3(n_pairs * hyp_blocks * slices), dim3(kThreads), 0, stream, kps_a, off_a, kps_b,
                       off_b, match, verified, pairs, n_hyp, hyp_blocks, slices, thr2, seed, counts);
    hipLaunchKernelGGL(fundamental_select, dim3(n_pairs), dim3(kThreads), 0, stream, kps_a, off_a, kps_b, off_b, match,
                       verified, pairs, counts, n_hyp, slices, thr2, seed, flags, F, stats);
}

}  // namespace lfmkd
