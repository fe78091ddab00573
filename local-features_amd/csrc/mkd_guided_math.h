// The admissibility tests of guided matching (mkd_match_guided.hip; contract: include/lf_mkd.h): the two verifiers' step-4
// inlier tests -- h_inlier() of mkd_homography_math.h under a homography, f_inlier() / sampson() of mkd_fundamental_math.h
// under a fundamental matrix -- in HOISTED form, every one __host__ __device__.  A matcher's workgroup tests one fixed point
// against many: what depends on one point alone is computed once for it and kept, the rest per pair of points.  Hoisting
// moves operations, it neither reorders nor re-associates one: each test below is the verifier's sequence of correctly
// rounded operations, operand for operand (the Sampson test's denominator stays ONE nested fma chain whose innermost two
// links depend on b alone), so a pair of points is admissible exactly when the verifier calls it an inlier, bit for bit.
// tests/cpp/guided_twin.cpp includes this header under a plain C++ compiler (with -ffp-contract=off) and is held to
// h_inlier() and f_inlier() themselves.  Needs <math.h> and <stdint.h> alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_verify_pair.h"   // the HIP qualifiers defined away without hipcc

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

// ---- homography: b ~ H a; inlier iff w > 0 and (bx w - u)^2 + (by w - v)^2 < thr^2 w^2 ---------------------------------
// what depends on a alone: the mapped point in homogeneous form and the right-hand side thr^2 w^2
struct GuideHA {
    float u, v, w, lim;
};
__host__ __device__ __forceinline__ GuideHA guide_h_of_a(const float *h, float ax, float ay, float thr2) {
    GuideHA r;
    r.u = fmaf(h[0], ax, fmaf(h[1], ay, h[2]));
    r.v = fmaf(h[3], ax, fmaf(h[4], ay, h[5]));
    r.w = fmaf(h[6], ax, fmaf(h[7], ay, h[8]));
    const float den = r.w * r.w;
    r.lim = thr2 * den;
    return r;
}
// ... and the test of b against it (b alone brings nothing to precompute)
__host__ __device__ __forceinline__ bool guide_h_test(const GuideHA &a, float bx, float by) {
    const float ex = fmaf(bx, a.w, -a.u), ey = fmaf(by, a.w, -a.v);
    const float num = fmaf(ex, ex, ey * ey);
    return a.w > 0.f && num < a.lim;
}

// ---- fundamental matrix: l = F a, l' = F^T b, e = b . l; inlier iff e^2 < thr^2 (l0^2 + l1^2 + l'0^2 + l'1^2) --------
// what depends on a alone: its epipolar line in b's image
struct GuideFA {
    float l0, l1, l2;
};
__host__ __device__ __forceinline__ GuideFA guide_f_of_a(const float *f, float ax, float ay) {
    GuideFA r;
    r.l0 = fmaf(f[0], ax, fmaf(f[1], ay, f[2]));
    r.l1 = fmaf(f[3], ax, fmaf(f[4], ay, f[5]));
    r.l2 = fmaf(f[6], ax, fmaf(f[7], ay, f[8]));
    return r;
}
// what depends on b alone: the point, and the inner two links of the denominator's chain, fmaf(m0, m0, m1 * m1)
struct GuideFB {
    float bx, by, mm;
};
__host__ __device__ __forceinline__ GuideFB guide_f_of_b(const float *f, float bx, float by) {
    GuideFB r;
    const float m0 = fmaf(f[0], bx, fmaf(f[3], by, f[6]));
    const float m1 = fmaf(f[1], bx, fmaf(f[4], by, f[7]));
    r.bx = bx;
    r.by = by;
    r.mm = fmaf(m0, m0, m1 * m1);
    return r;
}
__host__ __device__ __forceinline__ bool guide_f_test(const GuideFA &a, const GuideFB &b, float thr2) {
    const float e = fmaf(b.bx, a.l0, fmaf(b.by, a.l1, a.l2));
    const float num = e * e;
    const float den = fmaf(a.l0, a.l0, fmaf(a.l1, a.l1, b.mm));
    return num < thr2 * den;
}

// the two tests whole: is (a, b) admissible under the model?  kind: LF_MKD_GUIDE_HOMOGRAPHY 0, LF_MKD_GUIDE_FUNDAMENTAL 1
__host__ __device__ __forceinline__ bool guide_admissible(unsigned kind, const float *m, float ax, float ay, float bx, float by,
                                                          float thr2) {
    if (kind == 0u) return guide_h_test(guide_h_of_a(m, ax, ay, thr2), bx, by);
    return guide_f_test(guide_f_of_a(m, ax, ay), guide_f_of_b(m, bx, by), thr2);
}

}  // namespace
}  // namespace lfmkd
