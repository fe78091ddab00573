// gfx950 RANSAC homography verification of matches (lf_mkd_verify_homography*, include/lf_mkd.h).
//
// Three launches per call, whatever the number of pairs, none of which waits on another workgroup:
//
//   verify_prepare  one workgroup per pair: lists the pair's considered matches (0 <= match[i] < nb) by ascending i --
//                   the list is written into the caller's `verified` rows of that pair, which the last launch overwrites --
//                   and the per-pair normalisation (centroid, RMS distance sqrt(2)) of both point sets, into VerifyPair.
//   verify_score    the hot path.  One lane per hypothesis: it draws its 4 samples (counter-based sampler), solves the
//                   minimal problem in registers (square -> quad twice, H = B adj(A)), then walks the pair's rows, whose
//                   considered points the workgroup stages through LDS as float4 {ax, ay, bx, by} 256 rows at a time;
//                   every lane reads the same LDS address (a broadcast) and keeps its count in a register.  Grid =
//                   (pair, hypothesis block of 256, row slice): the slices (at most 16) split a pair's rows so that a call
//                   with few pairs still spreads over up to ~2 x CUs workgroups; each writes its partial counts.
//   verify_select   one workgroup per pair: argmax of the summed counts on the key (count, -k) by wave reductions, the
//                   winner's H recomputed by the same code, the least-squares refit (normal equations in f64, 8x8
//                   Cholesky in registers; a refit is kept if its truncated quadratic cost does not rise), the final
//                   rescoring, and H, verified, stats.
//
// What determines the bits: every step is a fixed sequence of IEEE operations -- this file is compiled with
// contraction OFF (the pragma below) and states its fused operations as fmaf -- so a hypothesis' H and every point's
// inlier test give the same bits in verify_score and verify_select, for any slicing of the rows, any number of pairs
// in the call, and any run.  Sums (normalisation f32, refit f64) run in a fixed per-thread order and a fixed tree.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mkd_verify_common.h"

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr int kMaxDraws = 32;                  // sampler draws per hypothesis
constexpr float kDegenerate = 1e-4f;           // |twice a triangle's area| below this in normalised coordinates

// Inlier test of one point under H (pixel coordinates, oriented so that the hypothesis' samples have w > 0):
// w > 0 and (bx w - u)^2 + (by w - v)^2 < thr^2 w^2, i.e. the forward transfer error below thr, without a division.
// `cost` receives the point's share of the truncated quadratic cost the refit is judged by: its squared transfer error if
// it is an inlier, else thr^2.
__device__ __forceinline__ bool inlier_cost(const float *h, float ax, float ay, float bx, float by, float thr2, float &cost) {
    const float u = fmaf(h[0], ax, fmaf(h[1], ay, h[2]));
    const float v = fmaf(h[3], ax, fmaf(h[4], ay, h[5]));
    const float w = fmaf(h[6], ax, fmaf(h[7], ay, h[8]));
    const float ex = fmaf(bx, w, -u), ey = fmaf(by, w, -v);
    const float num = fmaf(ex, ex, ey * ey), den = w * w;
    const bool in = w > 0.f && num < thr2 * den;
    cost = in ? num / den : thr2;
    return in;
}
__device__ __forceinline__ bool inlier(const float *h, float ax, float ay, float bx, float by, float thr2) {
    float unused;
    return inlier_cost(h, ax, ay, bx, by, thr2, unused);
}

__device__ __forceinline__ float cross3(float x0, float y0, float x1, float y1, float x2, float y2) {
    return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
}

// a quad is degenerate if any three of its points are (nearly) collinear or coincide
__device__ __forceinline__ bool quad_ok(const float *x, const float *y) {
    const float c0 = cross3(x[0], y[0], x[1], y[1], x[2], y[2]), c1 = cross3(x[0], y[0], x[1], y[1], x[3], y[3]);
    const float c2 = cross3(x[0], y[0], x[2], y[2], x[3], y[3]), c3 = cross3(x[1], y[1], x[2], y[2], x[3], y[3]);
    return fminf(fminf(fabsf(c0), fabsf(c1)), fminf(fabsf(c2), fabsf(c3))) >= kDegenerate;
}

// Heckbert's square -> quad map with the unit square's corners (0,0) (1,0) (1,1) (0,1) going to points 0..3, multiplied
// through by its denominator (no division, no affine special case): row-major 3x3
__device__ __forceinline__ void square_to_quad(const float *x, const float *y, float *m) {
    const float sx = x[0] - x[1] + x[2] - x[3], sy = y[0] - y[1] + y[2] - y[3];
    const float dx1 = x[1] - x[2], dx2 = x[3] - x[2], dy1 = y[1] - y[2], dy2 = y[3] - y[2];
    const float den = dx1 * dy2 - dx2 * dy1;
    const float g = sx * dy2 - dx2 * sy, hh = dx1 * sy - sx * dy1;
    m[0] = (x[1] - x[0]) * den + g * x[1];
    m[1] = (x[3] - x[0]) * den + hh * x[3];
    m[2] = x[0] * den;
    m[3] = (y[1] - y[0]) * den + g * y[1];
    m[4] = (y[3] - y[0]) * den + hh * y[3];
    m[5] = y[0] * den;
    m[6] = g;
    m[7] = hh;
    m[8] = den;
}

// H in normalised coordinates (b_n ~ Hn a_n) -> pixel coordinates: Tb^-1 Hn Ta; false if a value is not finite
__device__ __forceinline__ bool denormalise(const float *n, const VerifyPair &P, float *h) {
    float x[9];
    for (int r = 0; r < 3; ++r) {
        x[3 * r] = n[3 * r] * P.sa;
        x[3 * r + 1] = n[3 * r + 1] * P.sa;
        x[3 * r + 2] = n[3 * r + 2] - x[3 * r] * P.ca[0] - x[3 * r + 1] * P.ca[1];
    }
    const float ib = 1.f / P.sb;
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        h[c] = x[c] * ib + P.cb[0] * x[6 + c];
        h[3 + c] = x[3 + c] * ib + P.cb[1] * x[6 + c];
        h[6 + c] = x[6 + c];
    }
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(h[i]);
    return ok;
}

// Hypothesis k of pair p (include/lf_mkd.h, steps 2 and 3).  `list` = the pair's considered rows by position.
__device__ bool hypothesis(const float *ka, const float *kb, const int *match, const int *list, const VerifyPair &P,
                           unsigned seed_p, unsigned k, float *h) {
    const unsigned M = P.m;
    if (M < 4) return false;
    unsigned s0 = kInvalid, s1 = kInvalid, s2 = kInvalid, s3 = kInvalid;
    int got = 0;
    const uint64_t key = (uint64_t(seed_p) << 32) ^ (uint64_t(k) << 5);
    for (int t = 0; t < kMaxDraws && got < 4; ++t) {
        const uint64_t r = splitmix64(key ^ uint64_t(t));
        const unsigned pos = unsigned(((r >> 32) * uint64_t(M)) >> 32);
        if (pos == s0 || pos == s1 || pos == s2) continue;   // (s3 is still unset while drawing)
        s0 = got == 0 ? pos : s0;
        s1 = got == 1 ? pos : s1;
        s2 = got == 2 ? pos : s2;
        s3 = got == 3 ? pos : s3;
        ++got;
    }
    if (got < 4) return false;
    float ax[4], ay[4], bx[4], by[4];
    const unsigned s[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t r = uint64_t(unsigned(list[s[j]]));
        const uint64_t m = uint64_t(unsigned(match[r]));
        ax[j] = (ka[5 * r] - P.ca[0]) * P.sa;
        ay[j] = (ka[5 * r + 1] - P.ca[1]) * P.sa;
        bx[j] = (kb[5 * m] - P.cb[0]) * P.sb;
        by[j] = (kb[5 * m + 1] - P.cb[1]) * P.sb;
    }
    if (!quad_ok(ax, ay) || !quad_ok(bx, by)) return false;
    float A[9], B[9], J[9], n[9];
    square_to_quad(ax, ay, A);
    square_to_quad(bx, by, B);
    // adj(A): A^-1 up to a scale
    J[0] = A[4] * A[8] - A[5] * A[7];
    J[1] = A[2] * A[7] - A[1] * A[8];
    J[2] = A[1] * A[5] - A[2] * A[4];
    J[3] = A[5] * A[6] - A[3] * A[8];
    J[4] = A[0] * A[8] - A[2] * A[6];
    J[5] = A[2] * A[3] - A[0] * A[5];
    J[6] = A[3] * A[7] - A[4] * A[6];
    J[7] = A[1] * A[6] - A[0] * A[7];
    J[8] = A[0] * A[4] - A[1] * A[3];
    float big = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            n[3 * r + c] = B[3 * r] * J[c] + B[3 * r + 1] * J[3 + c] + B[3 * r + 2] * J[6 + c];
            big = fmaxf(big, fabsf(n[3 * r + c]));
        }
    if (!(big > 0.f) || !isfinite(big)) return false;
    const float ib = 1.f / big;
#pragma unroll
    for (int i = 0; i < 9; ++i) n[i] = n[i] * ib;
    // the samples' w must share one sign; H is oriented so that it is positive
    int pos = 0, neg = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float w = n[6] * ax[j] + n[7] * ay[j] + n[8];
        pos += w > 0.f;
        neg += w < 0.f;
    }
    if (pos != 4 && neg != 4) return false;
    if (neg == 4)
#pragma unroll
        for (int i = 0; i < 9; ++i) n[i] = -n[i];
    return denormalise(n, P, h);
}

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

// ---- launch 2: one lane per hypothesis, counts over a slice of the pair's rows ----------------------------------------
__global__ __launch_bounds__(kThreads) void verify_score(const float *kps_a, const uint64_t *off_a, const float *kps_b,
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
    float h[9];
    const bool valid = k < n_hyp && hypothesis(ka, kb, mt, list + oa, P, seed + p, k, h);
    unsigned count = 0;
    if (__syncthreads_or(valid)) {
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
                unsigned j = 0;
                for (; j + 4 <= n; j += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const f32x4 t = tile[j + u];
                        count += inlier(h, t.x, t.y, t.z, t.w, thr2);
                    }
                }
                for (; j < n; ++j) {
                    const f32x4 t = tile[j];
                    count += inlier(h, t.x, t.y, t.z, t.w, thr2);
                }
            }
            __syncthreads();
        }
    }
    if (k < n_hyp) counts[(uint64_t(p) * slices + sl) * n_hyp + k] = valid ? count : kInvalid;
}

// ---- launch 3: selection, refit, outputs ------------------------------------------------------------------------------
constexpr int kSums = 23;   // the distinct sums of the refit's normal equations

// the 23 moments of one inlier (normalised a = (x, y), b = (u, v); R = u^2 + v^2):
// xx xy yy x y 1 | uxx uxy uyy ux uy | vxx vxy vyy vx vy | Rxx Rxy Ryy | u v Rx Ry
__device__ __forceinline__ void add_moments(double *m, double x, double y, double u, double v) {
    const double xx = x * x, xy = x * y, yy = y * y, R = u * u + v * v;
    m[0] += xx; m[1] += xy; m[2] += yy; m[3] += x; m[4] += y; m[5] += 1.0;
    m[6] += u * xx; m[7] += u * xy; m[8] += u * yy; m[9] += u * x; m[10] += u * y;
    m[11] += v * xx; m[12] += v * xy; m[13] += v * yy; m[14] += v * x; m[15] += v * y;
    m[16] += R * xx; m[17] += R * xy; m[18] += R * yy;
    m[19] += u; m[20] += v; m[21] += R * x; m[22] += R * y;
}

// Least squares over the inliers with h8 = 1 in normalised coordinates: the 8x8 normal equations N h = r, solved by
// Cholesky (N is symmetric positive definite unless the inliers are degenerate: a pivot at or below 1e-12 of N's largest
// diagonal element fails the refit).  Every loop has constant bounds: the matrix stays in registers.
__device__ bool solve_refit(const double *m, float *n) {
    double N[8][8], r[8];
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) N[i][j] = 0.0;
    N[0][0] = N[3][3] = m[0]; N[0][1] = N[3][4] = m[1]; N[1][1] = N[4][4] = m[2];
    N[0][2] = N[3][5] = m[3]; N[1][2] = N[4][5] = m[4]; N[2][2] = N[5][5] = m[5];
    N[0][6] = -m[6]; N[0][7] = -m[7]; N[1][6] = -m[7]; N[1][7] = -m[8]; N[2][6] = -m[9]; N[2][7] = -m[10];
    N[3][6] = -m[11]; N[3][7] = -m[12]; N[4][6] = -m[12]; N[4][7] = -m[13]; N[5][6] = -m[14]; N[5][7] = -m[15];
    N[6][6] = m[16]; N[6][7] = m[17]; N[7][7] = m[18];
    r[0] = m[9]; r[1] = m[10]; r[2] = m[19]; r[3] = m[14]; r[4] = m[15]; r[5] = m[20]; r[6] = -m[21]; r[7] = -m[22];
    bool ok = cholesky8(N, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        n[i] = float(r[i]);
        ok = ok && isfinite(n[i]);
    }
    n[8] = 1.f;
    return ok;
}

__global__ __launch_bounds__(kThreads) void verify_select(const float *kps_a, const uint64_t *off_a, const float *kps_b,
                                                          const uint64_t *off_b, const int *match, int *verified,
                                                          const VerifyPair *pairs, const unsigned *counts, unsigned n_hyp,
                                                          unsigned slices, float thr2, unsigned seed, unsigned flags,
                                                          float *H_out, unsigned *stats) {
    __shared__ unsigned long long kred[kWaves];
    __shared__ double dred[kWaves * kSums];
    __shared__ unsigned ured[kWaves * 2];
    const unsigned p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t oa, ob;
    const uint64_t na = pair_rows(off_a, p, oa), nb = pair_rows(off_b, p, ob);
    const float *ka = kps_a + 5 * oa, *kb = kps_b + 5 * ob;
    const int *mt = match + oa;
    int *ver = verified + oa;
    const VerifyPair P = pairs[p];
    // argmax on (count, -k); an invalid hypothesis has key 0
    unsigned long long best = 0;
    const unsigned *cp = counts + uint64_t(p) * slices * n_hyp;
    for (unsigned k = tid; k < n_hyp; k += kThreads) {
        const unsigned c0 = cp[k];
        if (c0 == kInvalid) continue;
        // the slices' partial counts, 8 loads in flight at a time (a chain of single loads made this launch the call's cost)
        unsigned c = c0, s = 1;
        for (; s + 8 <= slices; s += 8) {
            unsigned v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = cp[uint64_t(s + j) * n_hyp + k];
#pragma unroll
            for (int j = 0; j < 8; ++j) c += v[j];
        }
        for (; s < slices; ++s) c += cp[uint64_t(s) * n_hyp + k];
        best = max(best, ((unsigned long long)(c + 1u) << 32) | (unsigned long long)(kInvalid - k));
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, o));
    if (lane == 0) kred[wave] = best;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) best = max(best, kred[w]);
    const bool found = best != 0;
    const unsigned k_best = found ? kInvalid - unsigned(best & 0xFFFFFFFFull) : kInvalid;
    const unsigned best_count = found ? unsigned(best >> 32) - 1u : 0u;
    // every thread recomputes the winner: the same bits as in verify_score
    float h[9];
    bool have = found && hypothesis(ka, kb, mt, verified + oa, P, seed + p, k_best, h);
    __syncthreads();   // the list of considered rows in `verified` has been read: from here on it is output
    unsigned final_count = 0;
    if (have) {
        const bool refine = !(flags & 1u);
        double m[kSums];
        unsigned n_cur = 0;
        double cost_cur = 0.0;
        for (int i = 0; i < kSums; ++i) m[i] = 0.0;
        for (uint64_t r = tid; r < na; r += kThreads) {
            Pt q;
            float e;
            if (!load_row(ka, kb, mt, r, nb, q)) continue;
            const bool in = inlier_cost(h, q.ax, q.ay, q.bx, q.by, thr2, e);
            cost_cur += e;
            if (!in) continue;
            ++n_cur;
            if (refine)
                add_moments(m, double((q.ax - P.ca[0]) * P.sa), double((q.ay - P.ca[1]) * P.sa), double((q.bx - P.cb[0]) * P.sb),
                            double((q.by - P.cb[1]) * P.sb));
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
            block_sum<double, kSums>(m, dred);
            float nh[9], h2[9];
            if (!solve_refit(m, nh) || !denormalise(nh, P, h2)) break;
            double m2[kSums];
            for (int i = 0; i < kSums; ++i) m2[i] = 0.0;
            unsigned c[2] = {0u, 0u};   // inliers of the refit, points whose membership changed
            double cost[1] = {0.0};     // the refit's truncated quadratic cost
            for (uint64_t r = tid; r < na; r += kThreads) {
                Pt q;
                float e;
                if (!load_row(ka, kb, mt, r, nb, q)) continue;
                const bool in_old = inlier(h, q.ax, q.ay, q.bx, q.by, thr2), in_new = inlier_cost(h2, q.ax, q.ay, q.bx, q.by, thr2, e);
                cost[0] += e;
                c[1] += in_old != in_new;
                if (!in_new) continue;
                ++c[0];
                add_moments(m2, double((q.ax - P.ca[0]) * P.sa), double((q.ay - P.ca[1]) * P.sa), double((q.bx - P.cb[0]) * P.sb),
                            double((q.by - P.cb[1]) * P.sb));
            }
            block_sum<unsigned, 2>(c, ured);
            block_sum<double, 1>(cost, dred);
            if (cost[0] > cost_cur) break;   // a refit whose truncated quadratic cost rises is not kept
            for (int i = 0; i < 9; ++i) h[i] = h2[i];
            for (int i = 0; i < kSums; ++i) m[i] = m2[i];
            n_cur = c[0];
            cost_cur = cost[0];
            if (c[1] == 0) break;      // the inlier set stopped changing
        }
        final_count = n_cur;
    }
    // outputs: verified (every row of the pair), H scaled to H[8] = 1, stats
    for (uint64_t r = tid; r < na; r += kThreads) {
        Pt q;
        const int m = mt[r];
        ver[r] = have && load_row(ka, kb, mt, r, nb, q) && inlier(h, q.ax, q.ay, q.bx, q.by, thr2) ? m : -1;
    }
    if (tid < 9) H_out[9 * uint64_t(p) + tid] = have ? h[tid] / h[8] : 0.f;
    if (tid < 4) {
        const unsigned st[4] = {have ? final_count : 0u, have ? best_count : 0u, have ? k_best : kInvalid, P.m};
        stats[4 * uint64_t(p) + tid] = tid == 0 ? st[0] : tid == 1 ? st[1] : tid == 2 ? st[2] : st[3];
    }
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
    if (n_pairs == 0) return;
    const float thr2 = threshold * threshold;
    const unsigned hyp_blocks = (n_hyp + kThreads - 1) / kThreads;
    launch_verify_prepare(kps_a, off_a, kps_b, off_b, match, n_pairs, pairs, verified, stream);
    hipLaunchKernelGGL(verify_score, dim3(n_pairs * hyp_blocks * slices), dim3(kThreads), 0, stream, kps_a, off_a, kps_b,
                       off_b, match, verified, pairs, n_hyp, hyp_blocks, slices, thr2, seed, counts);
    hipLaunchKernelGGL(verify_select, dim3(n_pairs), dim3(kThreads), 0, stream, kps_a, off_a, kps_b, off_b, match, verified,
                       pairs, counts, n_hyp, slices, thr2, seed, flags, H, stats);
}

}  // namespace lfmkd
