// The arithmetic of the RANSAC fundamental-matrix verifier (mkd_verify.hip; algorithm: include/lf_mkd.h): the sampler,
// the 7-point solver, the Sampson test and the refit's solve, every one __host__ __device__, and FundamentalModel, what
// ransac_score / ransac_select of mkd_verify.hip are instantiated with.  tests/cpp/fundamental_twin.cpp includes it under a
// plain C++ compiler (with -ffp-contract=off) and restates only the kernels' orchestration, so the host twin the device is held to bit for bit
// (tests/test_gpu_fundamental_exact.py) is this code and no transcription of it.  Needs <math.h> and <stdint.h> alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_verify_host.h"

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr int kMaxDraws = 64;                    // sampler draws per sample
constexpr float kPivotRel = 1e-5f;               // a Gauss-Jordan pivot at or below this times the first: invalid sample
constexpr float kLeadRel = 9.5367431640625e-7f;  // 2^-20: |c3| at or below this times max(|c0|, |c1|, |c2|): no candidate
constexpr int kBisect = 40;                      // bisection steps per bracketed root
constexpr int kNewton = 4;                       // Newton steps after them (a step leaving the bracket is not taken)
constexpr int kJacobiSweeps = 6;                 // cyclic Jacobi sweeps of the refit's rank-2 step
constexpr int kMoments = 36;                     // distinct moments b~_i b~_j a~_k a~_l of the refit's normal equations

// The 7 distinct positions of sample k (include/lf_mkd.h, step 2); false if 64 draws give fewer.
__host__ __device__ __forceinline__ bool sample7(unsigned seed_p, unsigned k, unsigned M, unsigned (&s)[7]) {
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = kInvalid;
    if (M < 7) return false;
    int got = 0;
    const uint64_t key = (uint64_t(seed_p) << 32) ^ (uint64_t(k) << 6);
    for (int t = 0; t < kMaxDraws && got < 7; ++t) {
        const uint64_t r = splitmix64(key ^ uint64_t(t));
        const unsigned pos = unsigned(((r >> 32) * uint64_t(M)) >> 32);
        bool dup = false;
#pragma unroll
        for (int i = 0; i < 7; ++i) dup = dup || pos == s[i];   // (unset entries are 0xFFFFFFFF > any position)
        if (dup) continue;
#pragma unroll
        for (int i = 0; i < 7; ++i) s[i] = got == i ? pos : s[i];
        ++got;
    }
    return got == 7;
}

// The two-dimensional null space of the 7 x 9 system A f = 0 (step 3): Gauss-Jordan elimination with full pivoting (the
// largest |entry| among the rows and columns not yet used, first in row-major order on a tie; every other row, used ones
// included, is eliminated with fmaf(-a * (1 / pivot), pivot row, row) and the pivot column set to exactly 0).  F1 and F2 are
// the null vectors with 1 in the first and the second unused column respectively and 0 in the other.  False if a pivot's
// magnitude is not above kPivotRel times the first pivot's.  Written with selects only: A stays in registers.
__host__ __device__ __forceinline__ bool null_space(float (&A)[7][9], float (&F1)[9], float (&F2)[9]) {
    unsigned used_r = 0, used_c = 0;
    int piv[7];
#pragma unroll
    for (int r = 0; r < 7; ++r) piv[r] = -1;
    float first = 0.f;
    bool ok = true;
#pragma unroll
    for (int step = 0; step < 7; ++step) {
        float best = -1.f;
        int pr = 0, pc = 0;
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const float v = fabsf(A[r][c]);
                const bool take = !((used_r >> r) & 1u) && !((used_c >> c) & 1u) && v > best;
                best = take ? v : best;
                pr = take ? r : pr;
                pc = take ? c : pc;
            }
        first = step == 0 ? best : first;
        ok = ok && best > kPivotRel * first;
        float P[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            float v = A[0][c];
#pragma unroll
            for (int r = 1; r < 7; ++r) v = r == pr ? A[r][c] : v;
            P[c] = v;
        }
        float pv = P[0];
#pragma unroll
        for (int c = 1; c < 9; ++c) pv = c == pc ? P[c] : pv;
        // (the sign goes onto the reciprocal and not onto the product: clang does not apply the contraction pragma to a unary
        // minus, and a negated product that met the column of ones -- fmaf(fct, 1, 1) folds to an addition -- was fused into
        // one fma on the device, which no host build does.  a * -inv is -(a * inv) exactly.)
        const float ninv = -(1.f / pv);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            float a = A[r][0];
#pragma unroll
            for (int c = 1; c < 9; ++c) a = c == pc ? A[r][c] : a;
            const float fct = a * ninv;
#pragma unroll
            for (int c = 0; c < 9; ++c) A[r][c] = r == pr ? A[r][c] : c == pc ? 0.f : fmaf(fct, P[c], A[r][c]);
        }
        used_r |= 1u << pr;
        used_c |= 1u << pc;
#pragma unroll
        for (int r = 0; r < 7; ++r) piv[r] = r == pr ? pc : piv[r];
    }
    int f1 = -1, f2 = -1;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const bool fr = !((used_c >> c) & 1u);
        f2 = fr && f1 >= 0 ? c : f2;
        f1 = fr && f1 < 0 ? c : f1;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        F1[c] = c == f1 ? 1.f : 0.f;
        F2[c] = c == f2 ? 1.f : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        float d = A[r][0], a1 = A[r][0], a2 = A[r][0];
#pragma unroll
        for (int c = 1; c < 9; ++c) {
            d = c == piv[r] ? A[r][c] : d;
            a1 = c == f1 ? A[r][c] : a1;
            a2 = c == f2 ? A[r][c] : a2;
        }
        const float nq = -(1.f / d);
        const float x1 = a1 * nq, x2 = a2 * nq;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            F1[c] = c == piv[r] ? x1 : F1[c];
            F2[c] = c == piv[r] ? x2 : F2[c];
        }
    }
    return ok;
}

// cofactor matrix of a row-major 3x3
__host__ __device__ __forceinline__ void cofactors(const float *m, float *c) {
    c[0] = m[4] * m[8] - m[5] * m[7];
    c[1] = m[5] * m[6] - m[3] * m[8];
    c[2] = m[3] * m[7] - m[4] * m[6];
    c[3] = m[2] * m[7] - m[1] * m[8];
    c[4] = m[0] * m[8] - m[2] * m[6];
    c[5] = m[1] * m[6] - m[0] * m[7];
    c[6] = m[1] * m[5] - m[2] * m[4];
    c[7] = m[2] * m[3] - m[0] * m[5];
    c[8] = m[0] * m[4] - m[1] * m[3];
}

__host__ __device__ __forceinline__ float dot9(const float *a, const float *b) {
    float s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) s = fmaf(a[i], b[i], s);
    return s;
}

__host__ __device__ __forceinline__ float cubic(float c0, float c1, float c2, float c3, float x) {
    return fmaf(fmaf(fmaf(c3, x, c2), x, c1), x, c0);
}

// Real roots of c3 x^3 + c2 x^2 + c1 x + c0, ascending, into x; returns how many (0 .. 3).  None if a coefficient is not
// finite or |c3| <= 2^-20 max(|c0|, |c1|, |c2|).  Every root lies in [-R, R], R = 1 + max(|c0|, |c1|, |c2|) / |c3|; the
// derivative's real roots e1 <= e2 (quadratic formula in its cancellation-free form, clamped to [-R, R]; both R if its
// discriminant c2^2 - 3 c3 c1 is not positive) cut [-R, R] into three monotone pieces.  A piece [lo, hi] holds a root iff
// (p(lo) < 0) != (p(hi) < 0); it is found by kBisect bisection steps that keep that property, from the midpoint of the last
// bracket, and kNewton Newton steps, a step that leaves the bracket (or is not a number) being skipped.
__host__ __device__ __forceinline__ int cubic_roots(float c0, float c1, float c2, float c3, float (&x)[3]) {
    const float big = fmaxf(fmaxf(fabsf(c0), fabsf(c1)), fabsf(c2));
    x[0] = x[1] = x[2] = 0.f;
    if (!(isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(c3)) || !(fabsf(c3) > kLeadRel * big)) return 0;
    const float R = 1.f + big / fabsf(c3);
    const float t = 3.f * c3;
    const float disc = fmaf(c2, c2, t * -c1);
    float e1 = R, e2 = R;
    if (disc > 0.f) {
        const float s = sqrtf(disc);
        const float q = -(c2 + copysignf(s, c2));
        const float r1 = q / t, r2 = c1 / q;
        e1 = fminf(fmaxf(fminf(r1, r2), -R), R);
        e2 = fminf(fmaxf(fmaxf(r1, r2), -R), R);
    }
    const float ends[4] = {-R, e1, e2, R};
    int n = 0;
#pragma unroll
    for (int piece = 0; piece < 3; ++piece) {
        float lo = ends[piece], hi = ends[piece + 1];
        const bool neg_lo = cubic(c0, c1, c2, c3, lo) < 0.f;
        if (neg_lo == (cubic(c0, c1, c2, c3, hi) < 0.f)) continue;
        for (int it = 0; it < kBisect; ++it) {
            const float m = (lo + hi) * 0.5f;
            const bool neg_m = cubic(c0, c1, c2, c3, m) < 0.f;
            lo = neg_m == neg_lo ? m : lo;
            hi = neg_m == neg_lo ? hi : m;
        }
        float r = (lo + hi) * 0.5f;
        for (int it = 0; it < kNewton; ++it) {
            const float d = fmaf(fmaf(t, r, 2.f * c2), r, c1);
            const float rn = r - cubic(c0, c1, c2, c3, r) / d;
            r = rn >= lo && rn <= hi ? rn : r;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) x[j] = n == j ? r : x[j];
        ++n;
    }
    return n;
}

// F in normalised coordinates (b_n^T Fn a_n = 0) -> pixel coordinates: Tb^T Fn Ta; false if a value is not finite
__host__ __device__ __forceinline__ bool f_denormalise(const float *n, const VerifyPair &P, float *f) {
    float x[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        x[3 * r] = n[3 * r] * P.sa;
        x[3 * r + 1] = n[3 * r + 1] * P.sa;
        x[3 * r + 2] = n[3 * r + 2] - x[3 * r] * P.ca[0] - x[3 * r + 1] * P.ca[1];
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f[c] = x[c] * P.sb;
        f[3 + c] = x[3 + c] * P.sb;
        f[6 + c] = x[6 + c] - P.cb[0] * f[c] - P.cb[1] * f[3 + c];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(f[i]);
    return ok;
}

// Sampson test of one point under F (pixel coordinates, step 4): l = F a, l' = F^T b, e = b . l; inlier iff
// e^2 < thr^2 (l0^2 + l1^2 + l'0^2 + l'1^2).  num and den receive e^2 and that sum.
__host__ __device__ __forceinline__ bool sampson(const float *f, float ax, float ay, float bx, float by, float thr2, float &num,
                                                 float &den) {
    const float l0 = fmaf(f[0], ax, fmaf(f[1], ay, f[2]));
    const float l1 = fmaf(f[3], ax, fmaf(f[4], ay, f[5]));
    const float l2 = fmaf(f[6], ax, fmaf(f[7], ay, f[8]));
    const float m0 = fmaf(f[0], bx, fmaf(f[3], by, f[6]));
    const float m1 = fmaf(f[1], bx, fmaf(f[4], by, f[7]));
    const float e = fmaf(bx, l0, fmaf(by, l1, l2));
    num = e * e;
    den = fmaf(l0, l0, fmaf(l1, l1, fmaf(m0, m0, m1 * m1)));
    return num < thr2 * den;
}
__host__ __device__ __forceinline__ bool f_inlier(const float *f, float ax, float ay, float bx, float by, float thr2) {
    float num, den;
    return sampson(f, ax, ay, bx, by, thr2, num, den);
}
// ... and the point's share of the MSAC cost: its Sampson error e^2 / sum if it is an inlier, else thr^2
__host__ __device__ __forceinline__ bool f_inlier_cost(const float *f, float ax, float ay, float bx, float by, float thr2,
                                                       float &cost) {
    float num, den;
    const bool in = sampson(f, ax, ay, bx, by, thr2, num, den);
    cost = in ? num / den : thr2;
    return in;
}

// Sample k of pair p (steps 2 and 3): up to three candidates, in ascending root order, in pixel coordinates (f) and in
// normalised coordinates scaled by their largest |entry| (fn).  Returns the valid candidates as bits 0..2 (a slot past the
// number of real roots, or whose scaling or pixel form is not finite, is invalid).  `list` = the pair's considered rows.
__host__ __device__ __forceinline__ unsigned candidates(const float *ka, const float *kb, const int *match, const int *list,
                                                        const VerifyPair &P, unsigned seed_p, unsigned k, float (&f)[3][9],
                                                        float (&fn)[3][9]) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 9; ++i) f[j][i] = fn[j][i] = 0.f;
    unsigned s[7];
    if (!sample7(seed_p, k, P.m, s)) return 0;
    float A[7][9];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const uint64_t r = uint64_t(unsigned(list[s[j]]));
        const uint64_t m = uint64_t(unsigned(match[r]));
        const float x = (ka[5 * r] - P.ca[0]) * P.sa, y = (ka[5 * r + 1] - P.ca[1]) * P.sa;
        const float u = (kb[5 * m] - P.cb[0]) * P.sb, v = (kb[5 * m + 1] - P.cb[1]) * P.sb;
        A[j][0] = u * x;
        A[j][1] = u * y;
        A[j][2] = u;
        A[j][3] = v * x;
        A[j][4] = v * y;
        A[j][5] = v;
        A[j][6] = x;
        A[j][7] = y;
        A[j][8] = 1.f;
    }
    float F1[9], F2[9];
    if (!null_space(A, F1, F2)) return 0;
    // det(l F1 + (1 - l) F2) = det(G + l D), G = F2, D = F1 - F2: c0 = det G, c1 = tr(adj(G) D), c2 = tr(adj(D) G), c3 = det D
    float D[9], CG[9], CD[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) D[i] = F1[i] - F2[i];
    cofactors(F2, CG);
    cofactors(D, CD);
    const float c0 = fmaf(F2[2], CG[2], fmaf(F2[1], CG[1], F2[0] * CG[0]));
    const float c3 = fmaf(D[2], CD[2], fmaf(D[1], CD[1], D[0] * CD[0]));
    const float c1 = dot9(CG, D), c2 = dot9(CD, F2);
    float lam[3];
    const int n = cubic_roots(c0, c1, c2, c3, lam);
    unsigned ok = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float g[9], big = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            g[i] = fmaf(lam[j], D[i], F2[i]);
            big = fmaxf(big, fabsf(g[i]));
        }
        bool good = j < n && big > 0.f && isfinite(big);
        const float ib = 1.f / big;
#pragma unroll
        for (int i = 0; i < 9; ++i) fn[j][i] = g[i] * ib;
        good = f_denormalise(fn[j], P, f[j]) && good;
        ok |= good ? 1u << j : 0u;
    }
    return ok;
}

// ---- the refit's pieces (step 5) ---------------------------------------------------------------------------------------
// The 36 moments of one inlier: b~ pairs {uu, uv, u, vv, v, 1} x a~ pairs {xx, xy, x, yy, y, 1}, index 6 * b_pair + a_pair
__host__ __device__ __forceinline__ void add_moments36(double *m, double x, double y, double u, double v) {
    const double a[6] = {x * x, x * y, x, y * y, y, 1.0};
    const double b[6] = {u * u, u * v, u, v * v, v, 1.0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int s = 0; s < 6; ++s) m[6 * q + s] += b[q] * a[s];
}

// index of the product of components i <= j of (u, v, 1) (or of (x, y, 1)) in {uu, uv, u, vv, v, 1}
__host__ __device__ constexpr int pair_index(int i, int j) { return i == 0 ? j : i == 1 ? 2 + j : 5; }

// element (i, j) of the 9x9 normal matrix sum r r^T, r = b~ (x) a~, f index 3 p + s for b component p and a component s
__host__ __device__ constexpr int normal_index(int i, int j) {
    return 6 * pair_index(i / 3 < j / 3 ? i / 3 : j / 3, i / 3 < j / 3 ? j / 3 : i / 3) +
           pair_index(i % 3 < j % 3 ? i % 3 : j % 3, i % 3 < j % 3 ? j % 3 : i % 3);
}

// Cyclic Jacobi on the symmetric 3x3 S (pairs (0,1) (0,2) (1,2), kJacobiSweeps sweeps, the textbook rotation:
// theta = (s_qq - s_pp) / (2 s_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), none where s_pq = 0); v = the eigenvector
// of the smallest diagonal element after it (the first on a tie).
__host__ __device__ __forceinline__ void smallest_eigenvector(double (&S)[3][3], double (&v)[3]) {
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = S[p][q];
            const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
            const double t0 = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double t = apq != 0.0 ? t0 : 0.0;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double kp = S[k][p], kq = S[k][q];
                S[k][p] = c * kp - s * kq;
                S[k][q] = s * kp + c * kq;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double pk = S[p][k], qk = S[q][k];
                S[p][k] = c * pk - s * qk;
                S[q][k] = s * pk + c * qk;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double kp = V[k][p], kq = V[k][q];
                V[k][p] = c * kp - s * kq;
                V[k][q] = s * kp + c * kq;
            }
        }
    }
    const int lo = S[1][1] < S[0][0] ? (S[2][2] < S[1][1] ? 2 : 1) : (S[2][2] < S[0][0] ? 2 : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = lo == 0 ? V[k][0] : lo == 1 ? V[k][1] : V[k][2];
}

// index of the largest |entry| of 9 (the first on a tie)
__host__ __device__ __forceinline__ int argmax_abs9(const float *x) {
    int c = 0;
    float b = fabsf(x[0]);
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const bool take = fabsf(x[i]) > b;
        b = take ? fabsf(x[i]) : b;
        c = take ? i : c;
    }
    return c;
}

// The 8x8 system of the refit with f_C = 1: the normal matrix without row and column C, and minus column C as its right-hand
// side.  C is a template argument so that every moment is read at a constant index (m stays in registers).
template <int C>
__host__ __device__ __forceinline__ void reduced_normal(const double *m, double (&N)[8][8], double (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int ii = i < C ? i : i + 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) N[i][j] = m[normal_index(ii, j < C ? j : j + 1)];
        r[i] = -m[normal_index(ii, C)];
    }
}

// Least squares over the moments' inliers with f_c = 1 in normalised coordinates (the other 8 unknowns by Cholesky), made
// rank 2 by F <- F (I - v v^T), scaled by its largest |entry| and rounded to f32 (fn); false if the Cholesky fails or a value
// is not finite.
__host__ __device__ __forceinline__ bool refit_solve(const double *m, int c, float (&fn)[9]) {
    double N[8][8], r[8];
    switch (c) {
    case 0: reduced_normal<0>(m, N, r); break;
    case 1: reduced_normal<1>(m, N, r); break;
    case 2: reduced_normal<2>(m, N, r); break;
    case 3: reduced_normal<3>(m, N, r); break;
    case 4: reduced_normal<4>(m, N, r); break;
    case 5: reduced_normal<5>(m, N, r); break;
    case 6: reduced_normal<6>(m, N, r); break;
    case 7: reduced_normal<7>(m, N, r); break;
    default: reduced_normal<8>(m, N, r); break;
    }
    bool ok = cholesky8(N, r);
    double F[3][3];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double v = 1.0;
        v = i < c ? r[i < 8 ? i : 7] : v;
        v = i > c ? r[i > 0 ? i - 1 : 0] : v;
        F[i / 3][i % 3] = v;
    }
    // rank 2: v = eigenvector of F^T F with the smallest eigenvalue
    double S[3][3], v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = F[0][i] * F[0][j] + F[1][i] * F[1][j] + F[2][i] * F[2][j];
    smallest_eigenvector(S, v);
    double G[9], big = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double w = F[i][0] * v[0] + F[i][1] * v[1] + F[i][2] * v[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            G[3 * i + j] = F[i][j] - w * v[j];
            big = fmax(big, fabs(G[3 * i + j]));
        }
    }
    ok = ok && big > 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        fn[i] = float(G[i] / big);
        ok = ok && isfinite(fn[i]);
    }
    return ok;
}

// What ransac_score / ransac_select (mkd_verify.hip) take from a model: see the list above them.
struct FundamentalModel {
    static constexpr int kCand = 3;        // a sample's cubic has up to three real roots
    static constexpr int kMoments = lfmkd::kMoments;
    static constexpr int kRows = 1;        // rows per unrolled scoring step
    __host__ __device__ static __forceinline__ unsigned candidates(const float *ka, const float *kb, const int *match,
                                                                   const int *list, const VerifyPair &P, unsigned seed_p,
                                                                   unsigned k, float (&f)[3][9], float (&fn)[3][9]) {
        return lfmkd::candidates(ka, kb, match, list, P, seed_p, k, f, fn);
    }
    __host__ __device__ static __forceinline__ bool inlier(const float *f, float ax, float ay, float bx, float by, float thr2) {
        return f_inlier(f, ax, ay, bx, by, thr2);
    }
    __host__ __device__ static __forceinline__ bool inlier_cost(const float *f, float ax, float ay, float bx, float by,
                                                                float thr2, float &cost) {
        return f_inlier_cost(f, ax, ay, bx, by, thr2, cost);
    }
    __host__ __device__ static __forceinline__ void add_moments(double *m, double x, double y, double u, double v) {
        add_moments36(m, x, y, u, v);
    }
    // (the current model's largest entry is the one the refit pins to 1)
    __host__ __device__ static __forceinline__ bool refit(const double *m, const float *fn, const VerifyPair &P, float (&fn2)[9],
                                                          float *f2) {
        return refit_solve(m, argmax_abs9(fn), fn2) && f_denormalise(fn2, P, f2);
    }
    // the entry the output is divided by: the one of largest magnitude
    __host__ __device__ static __forceinline__ float pivot(const float *f) {
        const int c = argmax_abs9(f);
        float piv = f[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) piv = i == c ? f[i] : piv;
        return piv;
    }
};

}  // namespace
}  // namespace lfmkd
