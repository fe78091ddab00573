// The arithmetic of the RANSAC homography verifier (mkd_verify.hip; algorithm: include/lf_mkd.h): the sampler, the
// four-point solver, the transfer-error test and the refit's solve, every one __host__ __device__, and HomographyModel, what
// ransac_score / ransac_select of mkd_verify.hip are instantiated with.  tests/cpp/guided_twin.cpp includes this header
// under a plain C++ compiler (with -ffp-contract=off) beside mkd_fundamental_math.h.  Needs <math.h> and <stdint.h> alone;
// the contraction pragma is here under mkd_verify_pair.h's rule (mkd_device.h must not include this file).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_verify_host.h"
#include "mkd_verify_pair.h"

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr int kHMaxDraws = 32;                 // sampler draws per hypothesis
constexpr float kDegenerate = 1e-4f;           // |twice a triangle's area| below this in normalised coordinates
constexpr int kSums = 23;                      // the distinct sums of the refit's normal equations

// Inlier test of one point under H (pixel coordinates, oriented so that the hypothesis' samples have w > 0):
// w > 0 and (bx w - u)^2 + (by w - v)^2 < thr^2 w^2, i.e. the forward transfer error below thr, without a division.
// `cost` receives the point's share of the truncated quadratic cost the refit is judged by: its squared transfer error if
// it is an inlier, else thr^2.
__host__ __device__ __forceinline__ bool h_inlier_cost(const float *h, float ax, float ay, float bx, float by, float thr2,
                                                       float &cost) {
    const float u = fmaf(h[0], ax, fmaf(h[1], ay, h[2]));
    const float v = fmaf(h[3], ax, fmaf(h[4], ay, h[5]));
    const float w = fmaf(h[6], ax, fmaf(h[7], ay, h[8]));
    const float ex = fmaf(bx, w, -u), ey = fmaf(by, w, -v);
    const float num = fmaf(ex, ex, ey * ey), den = w * w;
    const bool in = w > 0.f && num < thr2 * den;
    cost = in ? num / den : thr2;
    return in;
}
__host__ __device__ __forceinline__ bool h_inlier(const float *h, float ax, float ay, float bx, float by, float thr2) {
    float unused;
    return h_inlier_cost(h, ax, ay, bx, by, thr2, unused);
}

__host__ __device__ __forceinline__ float cross3(float x0, float y0, float x1, float y1, float x2, float y2) {
    return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
}

// a quad is degenerate if any three of its points are (nearly) collinear or coincide
__host__ __device__ __forceinline__ bool quad_ok(const float *x, const float *y) {
    const float c0 = cross3(x[0], y[0], x[1], y[1], x[2], y[2]), c1 = cross3(x[0], y[0], x[1], y[1], x[3], y[3]);
    const float c2 = cross3(x[0], y[0], x[2], y[2], x[3], y[3]), c3 = cross3(x[1], y[1], x[2], y[2], x[3], y[3]);
    return fminf(fminf(fabsf(c0), fabsf(c1)), fminf(fabsf(c2), fabsf(c3))) >= kDegenerate;
}

// Heckbert's square -> quad map with the unit square's corners (0,0) (1,0) (1,1) (0,1) going to points 0..3, multiplied
// through by its denominator (no division, no affine special case): row-major 3x3
__host__ __device__ __forceinline__ void square_to_quad(const float *x, const float *y, float *m) {
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
__host__ __device__ __forceinline__ bool h_denormalise(const float *n, const VerifyPair &P, float *h) {
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

// Hypothesis k of pair p (include/lf_mkd.h, steps 2 and 3), in normalised coordinates scaled by its largest |entry| (n) and
// in pixel coordinates (h).  `list` = the pair's considered rows by position.
__host__ __device__ __forceinline__ bool hypothesis(const float *ka, const float *kb, const int *match, const int *list,
                                                    const VerifyPair &P, unsigned seed_p, unsigned k, float *n, float *h) {
    const unsigned M = P.m;
    if (M < 4) return false;
    unsigned s0 = kInvalid, s1 = kInvalid, s2 = kInvalid, s3 = kInvalid;
    int got = 0;
    const uint64_t key = (uint64_t(seed_p) << 32) ^ (uint64_t(k) << 5);
    for (int t = 0; t < kHMaxDraws && got < 4; ++t) {
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
    float A[9], B[9], J[9];
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
    return h_denormalise(n, P, h);
}

// the 23 moments of one inlier (normalised a = (x, y), b = (u, v); R = u^2 + v^2):
// xx xy yy x y 1 | uxx uxy uyy ux uy | vxx vxy vyy vx vy | Rxx Rxy Ryy | u v Rx Ry
__host__ __device__ __forceinline__ void add_moments23(double *m, double x, double y, double u, double v) {
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
__host__ __device__ __forceinline__ bool h_solve_refit(const double *m, float *n) {
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

// What ransac_score / ransac_select (mkd_verify.hip) take from a model: see the list above them.
struct HomographyModel {
    static constexpr int kCand = 1;        // one hypothesis per sample
    static constexpr int kMoments = kSums;
    static constexpr int kRows = 4;        // rows per unrolled scoring step
    __host__ __device__ static __forceinline__ unsigned candidates(const float *ka, const float *kb, const int *match,
                                                                   const int *list, const VerifyPair &P, unsigned seed_p,
                                                                   unsigned k, float (&h)[1][9], float (&n)[1][9]) {
#pragma unroll
        for (int i = 0; i < 9; ++i) h[0][i] = n[0][i] = 0.f;
        return hypothesis(ka, kb, match, list, P, seed_p, k, n[0], h[0]) ? 1u : 0u;
    }
    __host__ __device__ static __forceinline__ bool inlier(const float *h, float ax, float ay, float bx, float by, float thr2) {
        return h_inlier(h, ax, ay, bx, by, thr2);
    }
    __host__ __device__ static __forceinline__ bool inlier_cost(const float *h, float ax, float ay, float bx, float by,
                                                                float thr2, float &cost) {
        return h_inlier_cost(h, ax, ay, bx, by, thr2, cost);
    }
    __host__ __device__ static __forceinline__ void add_moments(double *m, double x, double y, double u, double v) {
        add_moments23(m, x, y, u, v);
    }
    // (h8 = 1 whatever the current model: `n` is not read)
    __host__ __device__ static __forceinline__ bool refit(const double *m, const float *n, const VerifyPair &P, float *n2,
                                                          float *h2) {
        return h_solve_refit(m, n2) && h_denormalise(n2, P, h2);
    }
    // the entry the output is divided by
    __host__ __device__ static __forceinline__ float pivot(const float *h) { return h[8]; }
};

}  // namespace
}  // namespace lfmkd
