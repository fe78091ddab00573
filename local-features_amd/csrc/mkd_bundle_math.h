// The arithmetic of bundle adjustment (mkd_bundle.hip; algorithm: include/lf_mkd.h, lf_mkd_bundle_adjust_device): what an
// observation adds to its point's and its camera's normal equations, the coupling block W and its two products, the damping,
// the two solves, the conjugate-gradient scalars and the acceptance rule, every one __host__ __device__.
// tests/cpp/bundle_twin.cpp includes it under a plain C++ compiler (with -ffp-contract=off) and restates only the kernels'
// orchestration, so the host twin the device is held to bit for bit (tests/test_gpu_bundle.py) is this code and no
// transcription of it.  The camera rows, the 6x6 Cholesky solve, the Cayley update, the error and the 256-slot combine are
// mkd_resect_math.h's; the 3x3 cofactor solve, the 4-slot combine and the final inlier test are mkd_triangulate_math.h's.
// Everything is a fixed sequence of correctly rounded f64 operations (+ - * /, sqrt) under contraction OFF; no product is
// negated by a unary minus; no local array is indexed by a run-time value.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_resect_math.h"

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr unsigned kBaMaxIterations = 64, kBaMaxCg = 256;
constexpr double kBaDampFloor = 1e-6;                         // a diagonal entry d is damped by lambda max(d, this)
constexpr double kBaLambdaMin = 9.094947017729282379150390625e-13, kBaLambdaMax = 1099511627776.0;   // 2^-40, 2^40
constexpr int kBaPointTerms = 9;      // V00 V01 V02 V11 V12 V22, then g_p: tri_solve's layout
constexpr int kBaW = 18;              // W = J_c^T J_p, row-major [6][3]
constexpr int kBaTrace = 8;
constexpr unsigned long long kBaNoRow = ~0ull;
// flags of an image, a track and a position, as the kernels keep them in scratch
enum : unsigned { kBaCamUsable = 1, kBaCamFree = 2, kBaCamHeld = 4 };
enum : unsigned { kBaPointOk = 1, kBaPointFree = 2, kBaPointHeld = 4 };
enum : unsigned { kBaActive = 1, kBaCoupled = 2 };

using BaCorr = RsCorrT<double>;

// An observation at the current state: is it an inlier, its squared error, the camera's rows and the point's rows
// (a, 0, gx) R and (0, b, gy) R, written without the term that is zero.
struct BaLin {
    bool inlier;
    double e2;
    RsRows r;
    double px[3], py[3];
};
template <typename KT>
__host__ __device__ __forceinline__ void ba_rows(const RsPose &P, const KT *K, const BaCorr &c, BaLin &o) {
    rs_gn_rows(P, K, c, o.r);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.px[j] = o.r.a * P.R[j] + o.r.gx * P.R[6 + j];
        o.py[j] = o.r.b * P.R[3 + j] + o.r.gy * P.R[6 + j];
    }
}
template <typename KT>
__host__ __device__ __forceinline__ void ba_linearise(const RsPose &P, const KT *K, const BaCorr &c, double thr2, BaLin &o) {
    o.inlier = rs_inlier(P, K, c, thr2, o.e2);
    ba_rows(P, K, c, o);
}
// the nine values an inlier adds to its point: V's six distinct entries row by row, then g_p = J_p^T e
__host__ __device__ __forceinline__ void ba_point_terms(const BaLin &o, double *w) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) w[n++] = o.px[i] * o.px[j] + o.py[i] * o.py[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[6 + i] = o.px[i] * o.r.ex + o.py[i] * o.r.ey;
}
__host__ __device__ __forceinline__ void ba_coupling(const BaLin &o, double *W) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[3 * i + j] = o.r.Jx[i] * o.px[j] + o.r.Jy[i] * o.py[j];
}
// W^T v (v a camera's 6) and W y (y a point's 3), every sum left to right
__host__ __device__ __forceinline__ void ba_wt_v(const double *W, const double *v, double *o) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = W[j] * v[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) s = s + W[3 * i + j] * v[i];
        o[j] = s;
    }
}
__host__ __device__ __forceinline__ void ba_w_y(const double *W, const double *y, double *o) {
#pragma unroll
    for (int i = 0; i < 6; ++i) o[i] = W[3 * i] * y[0] + W[3 * i + 1] * y[1] + W[3 * i + 2] * y[2];
}

// Step 4: d + lambda max(d, 1e-6) on the diagonal of V (of the nine) and of U (of the 27)
__host__ __device__ __forceinline__ double ba_damp(double d, double lambda) { return d + lambda * (d > kBaDampFloor ? d : kBaDampFloor); }
__host__ __device__ __forceinline__ void ba_damp_v(double *w, double lambda) {
    w[0] = ba_damp(w[0], lambda);
    w[3] = ba_damp(w[3], lambda);
    w[5] = ba_damp(w[5], lambda);
}
__host__ __device__ __forceinline__ void ba_damp_u(double *w, double lambda) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        w[n] = ba_damp(w[n], lambda);
        n += 6 - i;
    }
}
// V*^-1 b by the triangulation call's cofactors, U*^-1 b by resection's Cholesky; false if singular / at a failed pivot
__host__ __device__ __forceinline__ bool ba_solve_v(const double *V, const double *b, double *x) {
    double w[kBaPointTerms];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = V[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[6 + i] = b[i];
    return tri_solve(w, x);
}
__host__ __device__ __forceinline__ bool ba_solve_u(const double *U, const double *b, double (&x)[6]) {
    double w[kRsTerms];
#pragma unroll
    for (int i = 0; i < 21; ++i) w[i] = U[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[21 + i] = b[i];
    return rs_cholesky6(w, x);
}
// U* p from the upper triangle, each row summed left to right
__host__ __device__ __forceinline__ void ba_u_times(const double *U, const double *p, double *o) {
    double N[6][6];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) N[i][j] = N[j][i] = U[n++];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = N[i][0] * p[0];
#pragma unroll
        for (int j = 1; j < 6; ++j) s = s + N[i][j] * p[j];
        o[i] = s;
    }
}
__host__ __device__ __forceinline__ double ba_dot6(const double *a, const double *b) {
    double s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) s = s + a[i] * b[i];
    return s;
}

// Step 5's scalars.  A step is: pAp -> ba_cg_alpha; x += alpha p, r -= alpha Ap, z = U*^-1 r; r.z -> ba_cg_beta; p = z + beta p.
struct BaCg {
    double rz, rz0, alpha, beta;
    unsigned stopped, steps;
};
__host__ __device__ __forceinline__ void ba_cg_start(BaCg &s, double rz0) {
    s.rz = s.rz0 = rz0;
    s.alpha = s.beta = 0.0;
    s.stopped = s.steps = 0;
}
__host__ __device__ __forceinline__ void ba_cg_alpha(BaCg &s, double pAp) {
    if (s.stopped) return;
    if (!(pAp > 0.0) || !(s.rz > 0.0)) {
        s.stopped = 1;
        return;
    }
    s.alpha = s.rz / pAp;
    s.steps += 1;
}
__host__ __device__ __forceinline__ void ba_cg_beta(BaCg &s, double rz, double tol2) {
    if (s.stopped) return;
    s.beta = rz / s.rz;
    s.rz = rz;
    if (!(rz > 0.0) || rz <= tol2 * s.rz0) s.stopped = 1;
}

// Step 6: accept iff the candidate is valid and cost' <= cost (a NaN fails); the next lambda
__host__ __device__ __forceinline__ bool ba_accept(double cost_new, double cost, double &lambda, bool valid = true) {
    const bool ok = valid && cost_new <= cost;
    const double down = lambda / 4.0, up = 8.0 * lambda;
    lambda = ok ? (down > kBaLambdaMin ? down : kBaLambdaMin) : (up < kBaLambdaMax ? up : kBaLambdaMax);
    return ok;
}

// Step 7: a state's pose rounded to f32 (rs_round without the intrinsics)
__host__ __device__ __forceinline__ void ba_round_pose(const RsPose &P, float *o) {
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = float(P.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[9 + i] = float(P.t[i]);
}

// ---- shared intrinsics (lf_mkd_bundle_adjust_intrinsics_device) -------------------------------------------------------------------
// A group of images taken with one lens has three parameters (s, dx, dy), (1, 0, 0) at the start: image i of the group has
// fx = s fx0_i, fy = s fy0_i, cx = cx0_i + dx, cy = cy0_i + dy.  The intrinsics the rows above read are then doubles; for an
// image of no free group they are the f32 values widened, whose bits under every function above are those of the float form.
constexpr int kBaTraceI = 9;          // the trace row of the intrinsics call: the eight above, then the held groups
constexpr int kBaGroupTerms = 9;      // U_kk's six distinct entries row by row, then g_k = J_k^T e: tri_solve's layout
constexpr int kBaCk = 18;             // U_ck = J_c^T J_k, row-major [6][3]: ba_w_y and ba_wt_v serve its two products
constexpr int kBaWk = 9;              // W_k = J_k^T J_p, row-major [3][3]
enum : unsigned { kBaRefineFocal = 1, kBaRefinePrincipal = 2 };
enum : unsigned { kBaGroupFree = 1, kBaGroupHeld = 2 };
enum : unsigned { kBaInlier = 4 };    // a position's third flag: an inlier at the iteration's state, whatever its camera

struct BaGroup {
    double s, dx, dy;
};
__host__ __device__ __forceinline__ void ba_widen_k(const float *K0, double *K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = double(K0[i]);
}
__host__ __device__ __forceinline__ void ba_group_k(const float *K0, const BaGroup &g, double *K) {
    K[0] = g.s * double(K0[0]);
    K[1] = g.s * double(K0[1]);
    K[2] = double(K0[2]) + g.dx;
    K[3] = double(K0[3]) + g.dy;
}
// The group's rows of an observation: d e_x / d (s, dx, dy) = (fx0 u, 1, 0), d e_y / d (s, dx, dy) = (fy0 v, 0, 1), a column
// that `refine` does not name being zero.
struct BaGRows {
    double jx[3], jy[3];
};
__host__ __device__ __forceinline__ void ba_group_rows(const BaLin &o, const float *K0, unsigned refine, BaGRows &g) {
    const bool f = (refine & kBaRefineFocal) != 0, c = (refine & kBaRefinePrincipal) != 0;
    g.jx[0] = f ? double(K0[0]) * o.r.u : 0.0;
    g.jy[0] = f ? double(K0[1]) * o.r.v : 0.0;
    g.jx[1] = c ? 1.0 : 0.0, g.jy[1] = 0.0;
    g.jx[2] = 0.0, g.jy[2] = c ? 1.0 : 0.0;
}
// the nine values an inlier adds to its group, the 18 of the block between its camera and its group, the nine between its
// group and its point
__host__ __device__ __forceinline__ void ba_group_terms(const BaLin &o, const BaGRows &g, double *w) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) w[n++] = g.jx[i] * g.jx[j] + g.jy[i] * g.jy[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[6 + i] = g.jx[i] * o.r.ex + g.jy[i] * o.r.ey;
}
__host__ __device__ __forceinline__ void ba_cross(const BaLin &o, const BaGRows &g, double *C) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = o.r.Jx[i] * g.jx[j] + o.r.Jy[i] * g.jy[j];
}
__host__ __device__ __forceinline__ void ba_coupling_k(const BaLin &o, const BaGRows &g, double *W) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[3 * i + j] = g.jx[i] * o.px[j] + g.jy[i] * o.py[j];
}
// W_k y and W_k^T v (3-vectors), every sum left to right
__host__ __device__ __forceinline__ void ba_wk_y(const double *W, const double *y, double *o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = W[3 * i] * y[0] + W[3 * i + 1] * y[1] + W[3 * i + 2] * y[2];
}
__host__ __device__ __forceinline__ void ba_wkt_v(const double *W, const double *v, double *o) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = W[j] * v[0] + W[3 + j] * v[1] + W[6 + j] * v[2];
}
// The group's damped block: ba_damp_v on the diagonal, then the rows and columns of the parameters `refine` does not name
// replaced by the identity's with a zero right-hand side, so that tri_solve serves and leaves them a zero step.  The
// identity's entry is not 1 but a damped diagonal entry of a refined parameter (s's for dx, dy; dx's for s): tri_solve's
// test compares the determinant with the cube of the mean diagonal, and a 1 beside a diagonal of 10^7 would fail it for
// every well-posed block.
__host__ __device__ __forceinline__ void ba_group_block(double *w, double lambda, unsigned refine) {
    ba_damp_v(w, lambda);
    const double s = w[0], c = w[3];
    if (!(refine & kBaRefineFocal)) w[0] = c, w[1] = 0.0, w[2] = 0.0, w[6] = 0.0;
    if (!(refine & kBaRefinePrincipal)) w[1] = 0.0, w[2] = 0.0, w[3] = s, w[4] = 0.0, w[5] = s, w[7] = 0.0, w[8] = 0.0;
}
// a 3-vector with the entries of the parameters `refine` does not name set to zero
__host__ __device__ __forceinline__ void ba_group_mask(double *v, unsigned refine) {
    if (!(refine & kBaRefineFocal)) v[0] = 0.0;
    if (!(refine & kBaRefinePrincipal)) v[1] = 0.0, v[2] = 0.0;
}
// U_kk* p from the six distinct entries, each row summed left to right
__host__ __device__ __forceinline__ void ba_v_times(const double *V, const double *p, double *o) {
    o[0] = V[0] * p[0] + V[1] * p[1] + V[2] * p[2];
    o[1] = V[1] * p[0] + V[3] * p[1] + V[4] * p[2];
    o[2] = V[2] * p[0] + V[4] * p[1] + V[5] * p[2];
}
__host__ __device__ __forceinline__ double ba_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// the candidate (s, dx, dy) - step, and whether it may be accepted: s finite and > 0
__host__ __device__ __forceinline__ bool ba_group_step(const BaGroup &g, const double *x, unsigned refine, BaGroup &o) {
    o = g;
    if (refine & kBaRefineFocal) o.s = g.s - x[0];
    if (refine & kBaRefinePrincipal) o.dx = g.dx - x[1], o.dy = g.dy - x[2];
    return pose_finite(o.s) && o.s > 0.0;
}
// Step 7: an image's intrinsics under its group's state, rounded to f32
__host__ __device__ __forceinline__ void ba_round_k(const float *K0, const BaGroup &g, float *o) {
    double K[4];
    ba_group_k(K0, g, K);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = float(K[i]);
}

}  // namespace
}  // namespace lfmkd
