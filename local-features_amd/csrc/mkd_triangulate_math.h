// The arithmetic of track triangulation (mkd_triangulate.hip; algorithm: include/lf_mkd.h, lf_mkd_triangulate_tracks_device):
// an observation's ray and its contribution to the midpoint system, the slot combine, the 3x3 solve, the inlier test and the
// parallax dot, every one __host__ __device__.  tests/cpp/triangulate_twin.cpp includes it under a plain C++ compiler (with
// -ffp-contract=off) and restates only what the kernel's group of lanes does with it, so the host twin the device is held to
// bit for bit (tests/test_gpu_triangulate.py) is this code and no transcription of it.  Needs <math.h> and <stdint.h> alone.
// Everything is a fixed sequence of correctly rounded f64 operations (+ - * /, sqrt) under contraction OFF; as in
// mkd_pose_math.h no product is negated by a unary minus: "0 - x" is written as a difference.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_pose_math.h"   // pose_finite, pose_ray

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

#ifndef LF_TRI_SLOTS
#define LF_TRI_SLOTS 4                     // (8 builds the A/B form of profiles/triangulate.md: another contract, the twin's too)
#endif
constexpr int kTriSlots = LF_TRI_SLOTS;    // slots of the canonical sum = lanes that own a track
static_assert(kTriSlots == 4 || kTriSlots == 8, "4, or 8 for the A/B build");
constexpr unsigned kTriCandidates = 8;     // the first usable positions that form the pair hypotheses
constexpr unsigned kTriRoundsMax = 4;
constexpr double kTriSingular = 1e-12;     // singular iff not (det > kTriSingular m^3), m the mean of the diagonal
constexpr unsigned kTriNoPair = 0xFFFFFFFFu;
constexpr int kTriTerms = 9;               // values of a contribution: P00 P01 P02 P11 P12 P22, (P c)0 1 2
enum : unsigned { kTriPoint = 0, kTriFewUsable = 1, kTriSingularSystem = 2, kTriFewInliers = 3 };

// What a usable position reads: the keypoint's x and y, its image's intrinsics and pose (R row-major, then t).
struct TriObs {
    float x, y, K[4], P[12];
};
// its unit ray in the world and its camera centre
struct TriRay {
    double u[3], c[3];
};

// the image half of "usable": finite intrinsics with fx, fy > 0, twelve finite pose values, R not all zero
__host__ __device__ __forceinline__ bool tri_camera_usable(const float *K, const float *P) {
    bool ok = true, any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) ok = ok && pose_finite(double(K[i]));
    ok = ok && K[0] > 0.f && K[1] > 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && pose_finite(double(P[i]));
#pragma unroll
    for (int i = 0; i < 9; ++i) any = any || P[i] != 0.f;
    return ok && any;
}
__host__ __device__ __forceinline__ bool tri_keypoint_usable(float x, float y) {
    return pose_finite(double(x)) && pose_finite(double(y));
}

// Step 1: d = R^T xn, u = d / sqrt(d.d), c = 0 - R^T t (every sum left to right).
__host__ __device__ __forceinline__ void tri_ray(const TriObs &o, TriRay &r) {
    double xn[3], d[3], R[9], t[3];
    pose_ray(o.x, o.y, o.K, xn);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = double(o.P[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = double(o.P[9 + i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = R[j] * xn[0] + R[3 + j] * xn[1] + R[6 + j] * xn[2];
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r.u[j] = d[j] / n;
        r.c[j] = 0.0 - (R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]);
    }
}

// the nine values a position adds: the six distinct entries of P = I - u u^T, then P c = c - u (u.c)
__host__ __device__ __forceinline__ void tri_contribution(const TriRay &r, double *w) {
    const double *u = r.u, *c = r.c;
    w[0] = 1.0 - u[0] * u[0];
    w[1] = 0.0 - u[0] * u[1];
    w[2] = 0.0 - u[0] * u[2];
    w[3] = 1.0 - u[1] * u[1];
    w[4] = 0.0 - u[1] * u[2];
    w[5] = 1.0 - u[2] * u[2];
    const double uc = u[0] * c[0] + u[1] * c[1] + u[2] * c[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) w[6 + j] = c[j] - u[j] * uc;
}

// Step 2's combine of the kTriSlots slot sums of ONE value: a butterfly over slot xor kTriSlots / 2 .. 2, 1, which for 4 is
// (s0 + s2) + (s1 + s3) (and for 8 ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7))).  (Addition commutes bit for bit, so every lane of the kernel's group
// ends with slot 0's value.)
__host__ __device__ __forceinline__ double tri_combine(const double *s) {
    double v[kTriSlots], w[kTriSlots];
#pragma unroll
    for (int j = 0; j < kTriSlots; ++j) v[j] = s[j];
#pragma unroll
    for (int m = kTriSlots / 2; m >= 1; m >>= 1) {
#pragma unroll
        for (int j = 0; j < kTriSlots; ++j) w[j] = v[j] + v[j ^ m];
#pragma unroll
        for (int j = 0; j < kTriSlots; ++j) v[j] = w[j];
    }
    return v[0];
}

// Step 3: A X = b by cofactors, A = (a00 a01 a02 a11 a12 a22) = w[0..5], b = w[6..8].  False if singular (a NaN included).
__host__ __device__ __forceinline__ bool tri_solve(const double *w, double *X) {
    const double a00 = w[0], a01 = w[1], a02 = w[2], a11 = w[3], a12 = w[4], a22 = w[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double m = (a00 + a11 + a22) / 3.0;
    X[0] = (c00 * w[6] + c01 * w[7] + c02 * w[8]) / det;
    X[1] = (c01 * w[6] + c11 * w[7] + c12 * w[8]) / det;
    X[2] = (c02 * w[6] + c12 * w[7] + c22 * w[8]) / det;
    return det > kTriSingular * (m * m * m);
}

// Step 4: the squared reprojection error of X in a usable position; false if X is not in front (p_z > 0 fails).
__host__ __device__ __forceinline__ bool tri_error2(const TriObs &o, const double *X, double &e2) {
    double p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        p[r] = double(o.P[3 * r]) * X[0] + double(o.P[3 * r + 1]) * X[1] + double(o.P[3 * r + 2]) * X[2] + double(o.P[9 + r]);
    const double ex = double(o.K[0]) * (p[0] / p[2]) + double(o.K[2]) - double(o.x);
    const double ey = double(o.K[1]) * (p[1] / p[2]) + double(o.K[3]) - double(o.y);
    e2 = ex * ex + ey * ey;
    return p[2] > 0.0;
}
__host__ __device__ __forceinline__ bool tri_inlier(const TriObs &o, const double *X, double thr2, double &e2) {
    const bool front = tri_error2(o, X, e2);
    return front && e2 <= thr2;
}

// Step 7: the cosine between two rays; 2 ("none") where it is a NaN, so that a minimum over it has one answer in any order.
__host__ __device__ __forceinline__ double tri_cosine(const double *a, const double *b) {
    const double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    return d == d ? d : 2.0;
}
// is (v, position) before (w, position): the smaller value, the lower position on a tie
__host__ __device__ __forceinline__ bool tri_before(double v, uint64_t pv, double w, uint64_t pw) {
    return v < w || (v == w && pv < pw);
}

}  // namespace
}  // namespace lfmkd
