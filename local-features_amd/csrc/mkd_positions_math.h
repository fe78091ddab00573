// The arithmetic of the tree-pose and global-positioning calls (mkd_positions.hip; algorithm: include/lf_mkd.h,
// lf_mkd_tree_poses_device and lf_mkd_global_positions_device): the unit step of a tree edge, an observation's world ray, its
// robust weight, its weighted contribution to a point's or a camera's 3x3 system, the decision of a solve, the residual, the
// gauge transform and the translation of a centre, every one __host__ __device__.  tests/cpp/positions_twin.cpp includes it
// under a plain C++ compiler (with -ffp-contract=off) and restates only what the kernels do with it, so the host twin the
// device is held to bit for bit (tests/test_gpu_positions.py) is this code and no transcription of it.  The ray is tri_ray's,
// the contribution tri_contribution's and the solve tri_solve's, called here; the 4-slot and 256-slot sums are the orders
// tri_combine and rs_combine define, which the twin calls and the kernels form with lane butterflies as their siblings do.  Needs <math.h> and <stdint.h> alone.  Everything is a fixed sequence of
// correctly rounded f64 operations (+ - * /, sqrt) under contraction OFF; no product is negated by a unary minus.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_resect_math.h"   // rs_combine, kRsSlots; TriObs, tri_ray, tri_contribution, tri_combine, tri_solve through it

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr unsigned kGpNone = 0xFFFFFFFFu;
constexpr int kGpTerms = kTriTerms;         // w P's six distinct entries, then w P y: tri_solve's layout
// a camera's (d_image_stats word 3) or a point's latest step
enum : unsigned { kGpSolved = 0, kGpNotRegistered = 1, kGpFewObservations = 2, kGpSingular = 3 };
// d_counts' words
enum : int { kGpCRegistered = 0, kGpCSolvedPoints, kGpCUsable, kGpCWeighted, kGpCHeld, kGpCGaugeFailed, kGpCTracks, kGpCSweeps };

__host__ __device__ __forceinline__ bool gp_finite3(const double *v) {
    return pose_finite(v[0]) && pose_finite(v[1]) && pose_finite(v[2]);
}

// ---- tree poses ---------------------------------------------------------------------------------------------------------------
// The step of tree edge (a, b) with translation t (x_b = R x_a + t): d = 0 - R_b^T t is parallel to c_b - c_a; u = d / |d|.
// False if t or R_b is not finite or d has no length.
__host__ __device__ __forceinline__ bool gp_tree_step(const float *Rb, const float *t, double *u) {
    double d[3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && pose_finite(double(Rb[i]));
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && pose_finite(double(t[i]));
#pragma unroll
    for (int j = 0; j < 3; ++j)
        d[j] = 0.0 - (double(Rb[j]) * double(t[0]) + double(Rb[3 + j]) * double(t[1]) + double(Rb[6 + j]) * double(t[2]));
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = d[j] / n;
    return ok && n > 0.0 && gp_finite3(u);
}
__host__ __device__ __forceinline__ bool gp_rotation_set(const float *R) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) any = any || R[i] != 0.f;
    return any;
}
// t = 0 - R c, rounded once to f32
__host__ __device__ __forceinline__ void gp_translation(const float *R, const double *c, float *t) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        t[r] = float(0.0 - (double(R[3 * r]) * c[0] + double(R[3 * r + 1]) * c[1] + double(R[3 * r + 2]) * c[2]));
}

// ---- global positions ---------------------------------------------------------------------------------------------------------
// the observation record of a keypoint under rotation R alone (t = 0): what tri_ray reads
__host__ __device__ __forceinline__ TriObs gp_obs(float x, float y, const float *K, const float *R) {
    TriObs o;
    o.x = x, o.y = y;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.K[i] = K[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) o.P[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.P[9 + i] = 0.f;
    return o;
}
// the world ray v = R^T f / |f| of a keypoint (tri_ray's u)
__host__ __device__ __forceinline__ void gp_ray(float x, float y, const float *K, const float *R, double *v) {
    TriRay r;
    tri_ray(gp_obs(x, y, K, R), r);
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = r.u[j];
}
// the centre 0 - R^T t of a pose (tri_ray's c)
__host__ __device__ __forceinline__ void gp_centre(const float *K, const float *P, double *c) {
    TriObs o = gp_obs(0.f, 0.f, K, P);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.P[9 + i] = P[9 + i];
    TriRay r;
    tri_ray(o, r);
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = r.c[j];
}

// |P r|^2 and |r|^2 and v . r of r = X - c under P = I - v v^T
__host__ __device__ __forceinline__ void gp_residual(const double *v, const double *X, const double *c, double &pr2, double &rr,
                                                     double &depth) {
    const double r[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
    depth = v[0] * r[0] + v[1] * r[1] + v[2] * r[2];
    const double p[3] = {r[0] - v[0] * depth, r[1] - v[1] * depth, r[2] - v[2] * depth};
    pr2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}
// The weight: 1 while `robust` is off.  Else 0 if the point is not in front (v . r <= 0), r is zero or anything is not
// finite; else s0 / max(s, s0) with s = sqrt(|P r|^2 / |r|^2), the sine of the angle between the ray and r.
__host__ __device__ __forceinline__ double gp_weight(const double *v, const double *X, const double *c, double s0, bool robust) {
    if (!robust) return 1.0;
    double pr2, rr, depth;
    gp_residual(v, X, c, pr2, rr, depth);
    if (!(depth > 0.0) || !(rr > 0.0) || !pose_finite(pr2) || !pose_finite(rr)) return 0.0;
    const double s = sqrt(pr2 / rr);
    if (!pose_finite(s)) return 0.0;
    return s > s0 ? s0 / s : 1.0;
}
// the nine values w P (six distinct entries) and w P y an observation adds to the system of the unknown opposite y
__host__ __device__ __forceinline__ void gp_terms(const double *v, double w, const double *y, double *out) {
    TriRay r;
#pragma unroll
    for (int j = 0; j < 3; ++j) r.u[j] = v[j], r.c[j] = y[j];
    tri_contribution(r, out);
#pragma unroll
    for (int k = 0; k < kGpTerms; ++k) out[k] = w * out[k];
}
// the decision of a step from its combined sums and the number of observations with w > 0: the solution in X if kGpSolved
__host__ __device__ __forceinline__ unsigned gp_solve(const double *sums, unsigned weighted, unsigned min_obs, double *X) {
    const bool ok = tri_solve(sums, X) && gp_finite3(X);
    return weighted < min_obs ? kGpFewObservations : ok ? kGpSolved : kGpSingular;
}
// (x - m) / rho
__host__ __device__ __forceinline__ void gp_regauge(double *x, const double *m, double rho) {
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = (x[j] - m[j]) / rho;
}
// the state of an observation from its final weight
__host__ __device__ __forceinline__ unsigned gp_state(bool usable, bool solved, double w) {
    return !usable ? 0u : solved && w >= 0.5 ? 2u : 1u;
}

}  // namespace
}  // namespace lfmkd
