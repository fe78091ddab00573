// The arithmetic of camera resection (mkd_resect.hip; algorithm: include/lf_mkd.h, lf_mkd_resect_cameras_device): the
// candidate and correspondence rules, the bearing, the 3-position sampler, Grunert's P3P quartic with its fixed-iteration real
// root finder, the pose of a root, the inlier test of an f64 pose, the Gauss-Newton terms, the 6x6 Cholesky solve, the Cayley
// update and the combine of the 256-slot canonical sum, every one __host__ __device__.  tests/cpp/resect_twin.cpp includes it
// under a plain C++ compiler (with -ffp-contract=off) and restates only the three kernels' orchestration, so the host twin the
// device is held to bit for bit (tests/test_gpu_resect.py) is this code and no transcription of it.  Needs <math.h> and
// <stdint.h> alone.  Everything is a fixed sequence of correctly rounded f64 operations (+ - * /, sqrt) under contraction OFF;
// as in mkd_pose_math.h no product is negated by a unary minus: "0 - x" is written as a difference.  No local array is
// indexed by a run-time value (every loop over one has constant bounds and is unrolled; a run-time pick is a chain of
// selects), so the kernels keep everything in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_triangulate_math.h"   // TriObs, tri_inlier; pose_finite, pose_ray through it
#include "mkd_verify_host.h"        // splitmix64

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr int kRsSlots = 256;               // slots of the canonical sum = threads of a workgroup
constexpr unsigned kRsMaxSamples = 4096;
constexpr unsigned kRsRoundsMax = 4;
constexpr int kRsMaxDraws = 64;             // sampler draws per sample
constexpr int kRsBisect = 64;               // bisection steps per bracketed root: the bracket is at most 2^22 wide (kRsLeadRel),
                                            // so 2^-42 after them
constexpr int kRsNewton = 4;                // guarded Newton steps after them: 2^-42 squares to below an ulp in two, two to spare
// invalid sample iff not (|(X2 - X1) x (X3 - X1)|^2 > kRsCollinear |X2 - X1|^2 |X3 - X1|^2): a guard against exactly degenerate
// triangles (it is sin^2 of the angle at X1, so it trips below about 1e-6 rad), not a quality gate -- the inlier count is.
constexpr double kRsCollinear = 1e-12;
// invalid sample iff not (|A4| > kRsLeadRel max |A0 .. A3|), 2^-20 as the F verifier's cubic: a vanishing leading coefficient
// sends a root to infinity and the Cauchy bound with it; it also bounds the bracket the bisection count is sized for.
constexpr double kRsLeadRel = 9.5367431640625e-7;
constexpr unsigned kRsNone = 0xFFFFFFFFu;
constexpr int kRsTerms = 27;                // the refit's sums: 21 of J^T J's upper triangle, row by row, then 6 of J^T e
enum : unsigned { kRsPose = 0, kRsNotCandidate = 1, kRsNoCandidate = 2, kRsFewInliers = 3 };

// a correspondence: the keypoint and its track's point (T = float as the arrays hold it; bundle adjustment's f64 state reads
// the same functions with T = double, where the widening double(c.X) is the identity)
template <typename T>
struct RsCorrT {
    float x, y;
    T X, Y, Z;
};
using RsCorr = RsCorrT<float>;
struct RsPose {
    double R[9], t[3];
};

// Image i is a CANDIDATE iff its intrinsics are finite with fx, fy > 0, its 12 pose values are finite, and R is all zero or
// `all` is set.
__host__ __device__ __forceinline__ bool rs_candidate(const float *K, const float *P, bool all) {
    bool ok = true, any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) ok = ok && pose_finite(double(K[i]));
    ok = ok && K[0] > 0.f && K[1] > 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && pose_finite(double(P[i]));
#pragma unroll
    for (int i = 0; i < 9; ++i) any = any || P[i] != 0.f;
    return ok && (all || !any);
}
// the point half of "correspondence": finite X, Y, Z and w <= cmin (a NaN fails)
__host__ __device__ __forceinline__ bool rs_point_usable(const float *p, double cmin) {
    return pose_finite(double(p[0])) && pose_finite(double(p[1])) && pose_finite(double(p[2])) && double(p[3]) <= cmin;
}

// Step 1: f = xn / sqrt(xn.xn), xn = ((x - cx) / fx, (y - cy) / fy, 1).
__host__ __device__ __forceinline__ void rs_bearing(float x, float y, const float *K, double *f) {
    double xn[3];
    pose_ray(x, y, K, xn);
    const double n = sqrt(xn[0] * xn[0] + xn[1] * xn[1] + xn[2] * xn[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = xn[i] / n;
}

// Step 2: the 3 distinct positions of sample k of image `seed_i` = seed + image id; false if M < 3 or 64 draws give fewer.
__host__ __device__ __forceinline__ bool sample3(unsigned seed_i, unsigned k, unsigned M, unsigned (&s)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) s[i] = kRsNone;
    if (M < 3) return false;
    int got = 0;
    const uint64_t key = (uint64_t(seed_i) << 32) ^ (uint64_t(k) << 6);
    for (int t = 0; t < kRsMaxDraws && got < 3; ++t) {
        const uint64_t r = splitmix64(key ^ uint64_t(t));
        const unsigned pos = unsigned(((r >> 32) * uint64_t(M)) >> 32);
        bool dup = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) dup = dup || pos == s[i];   // (unset entries are 0xFFFFFFFF > any position)
        if (dup) continue;
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = got == i ? pos : s[i];
        ++got;
    }
    return got == 3;
}

// a[0] + a[1] x + .. + a[N] x^N by Horner
template <int N>
__host__ __device__ __forceinline__ double rs_poly(const double (&a)[N + 1], double x) {
    double v = a[N];
#pragma unroll
    for (int i = N - 1; i >= 0; --i) v = v * x + a[i];
    return v;
}

// The real roots of a polynomial of degree N (2 .. 4, a[N] != 0) inside [-B, B], ascending; returns their number, the unused
// entries of r are B.  N = 2 in closed form (q = -(b + sign(b) sqrt(disc)) / 2, the roots q / a and c / q; none iff not
// disc >= 0).  N > 2: the breakpoints are -B, the derivative's real roots (this function at N - 1, clamped to [-B, B]) and B;
// an interval (lo, hi) with lo < hi holds a root iff (p(lo) > 0) != (p(hi) > 0); it is halved kRsBisect times (mid = (lo +
// hi) / 2 replaces the end whose sign it has), x = the last interval's middle, then kRsNewton times x' = x - p(x) / p'(x),
// taken iff lo <= x' <= hi.  (A root of even multiplicity is found twice or not at all: no interval's ends differ in sign by
// it alone.)
template <int N>
__host__ __device__ __forceinline__ int rs_real_roots(const double (&a)[N + 1], double B, double (&r)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = B;
    if constexpr (N == 2) {
        const double disc = a[1] * a[1] - 4.0 * a[2] * a[0];
        if (!(disc >= 0.0)) return 0;
        const double s = sqrt(disc);
        const double q = a[1] < 0.0 ? (s - a[1]) * 0.5 : (0.0 - (a[1] + s)) * 0.5;
        const double x1 = q / a[2], x2 = q != 0.0 ? a[0] / q : x1;
        r[0] = x1 < x2 ? x1 : x2;
        r[1] = x1 < x2 ? x2 : x1;
        return 2;
    } else {
        double d[N], cr[N - 1], brk[N + 1];
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = double(i + 1) * a[i + 1];
        rs_real_roots<N - 1>(d, B, cr);
        const double nB = 0.0 - B;
        brk[0] = nB;
        brk[N] = B;
#pragma unroll
        for (int i = 0; i < N - 1; ++i) brk[i + 1] = cr[i] < nB ? nB : cr[i] > B ? B : cr[i];
        int n = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double lo = brk[i], hi = brk[i + 1];
            const bool up = rs_poly<N>(a, hi) > 0.0;
            if (!(lo < hi) || (rs_poly<N>(a, lo) > 0.0) == up) continue;
            for (int it = 0; it < kRsBisect; ++it) {
                const double mid = (lo + hi) * 0.5;
                const bool m = rs_poly<N>(a, mid) > 0.0;
                hi = m == up ? mid : hi;
                lo = m == up ? lo : mid;
            }
            double x = (lo + hi) * 0.5;
            for (int it = 0; it < kRsNewton; ++it) {
                const double xn = x - rs_poly<N>(a, x) / rs_poly<N - 1>(d, x);
                x = xn >= lo && xn <= hi ? xn : x;
            }
#pragma unroll
            for (int j = 0; j < N; ++j) r[j] = n == j ? x : r[j];
            ++n;
        }
        return n;
    }
}

// What step 3 keeps of a sample: the quartic and what a root's pose needs.
struct RsP3P {
    double f[3][3], X[3][3];        // bearings, world points
    double b2, ca, cb, cg, p;       // |X1 - X3|^2, the cosines, (a^2 - c^2) / b^2
    double A[5], B;                 // A[i] x^i, the Cauchy bound 1 + max |A0 .. A3| / |A4|
};

__host__ __device__ __forceinline__ double rs_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ __forceinline__ void rs_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// Step 3, the quartic of a sample (s[0], s[1], s[2] are X1, X2, X3 with their keypoints).  False if the sample is invalid: the
// triangle (nearly) collinear, the leading coefficient vanishing against the others, or a coefficient not finite.
__host__ __device__ __forceinline__ bool rs_p3p_quartic(const RsCorr (&s)[3], const float *K, RsP3P &q) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rs_bearing(s[i].x, s[i].y, K, q.f[i]);
        q.X[i][0] = double(s[i].X);
        q.X[i][1] = double(s[i].Y);
        q.X[i][2] = double(s[i].Z);
    }
    double d12[3], d13[3], d23[3], cr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d12[i] = q.X[1][i] - q.X[0][i];
        d13[i] = q.X[2][i] - q.X[0][i];
        d23[i] = q.X[2][i] - q.X[1][i];
    }
    const double a2 = rs_dot(d23, d23), b2 = rs_dot(d13, d13), c2 = rs_dot(d12, d12);
    rs_cross(d12, d13, cr);
    bool ok = rs_dot(cr, cr) > kRsCollinear * (c2 * b2);
    const double ca = rs_dot(q.f[1], q.f[2]), cb = rs_dot(q.f[0], q.f[2]), cg = rs_dot(q.f[0], q.f[1]);
    const double p = (a2 - c2) / b2, qq = (a2 + c2) / b2, rc = c2 / b2, ra = a2 / b2;
    const double pm = p - 1.0, pp = 1.0 + p, oq = 1.0 - qq;
    q.A[4] = pm * pm - 4.0 * rc * (ca * ca);
    q.A[3] = 4.0 * ((p * (1.0 - p) * cb - oq * ca * cg) + 2.0 * rc * (ca * ca) * cb);
    q.A[2] = 2.0 * (((((p * p - 1.0) + 2.0 * (p * p) * (cb * cb)) + 2.0 * ((b2 - c2) / b2) * (ca * ca)) - 4.0 * qq * ca * cb * cg) +
                    2.0 * ((b2 - a2) / b2) * (cg * cg));
    q.A[1] = 4.0 * ((2.0 * ra * (cg * cg) * cb - p * pp * cb) - oq * ca * cg);
    q.A[0] = pp * pp - 4.0 * ra * (cg * cg);
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double m = fabs(q.A[i]);
        big = m > big ? m : big;
        ok = ok && pose_finite(q.A[i]);
    }
    const double lead = fabs(q.A[4]);
    ok = ok && pose_finite(q.A[4]) && lead > kRsLeadRel * big;
    q.B = 1.0 + big / lead;
    q.b2 = b2;
    q.ca = ca;
    q.cb = cb;
    q.cg = cg;
    q.p = p;
    return ok;
}

// the orthonormal frame of a triangle as columns e1, e2, e3 (F[r][k] = e_k's component r)
__host__ __device__ __forceinline__ void rs_frame(const double *P1, const double *P2, const double *P3, double (&F)[3][3]) {
    double d12[3], d13[3], e1[3], e2[3], e3[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d12[i] = P2[i] - P1[i];
        d13[i] = P3[i] - P1[i];
    }
    const double n1 = sqrt(rs_dot(d12, d12));
#pragma unroll
    for (int i = 0; i < 3; ++i) e1[i] = d12[i] / n1;
    rs_cross(e1, d13, c);
    const double n3 = sqrt(rs_dot(c, c));
#pragma unroll
    for (int i = 0; i < 3; ++i) e3[i] = c[i] / n3;
    rs_cross(e3, e1, e2);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        F[i][0] = e1[i];
        F[i][1] = e2[i];
        F[i][2] = e3[i];
    }
}

// Step 3, the pose of a real root v.  False (the candidate is skipped) unless v > 0, the denominator of u is not 0, u > 0 and
// all twelve values of the pose are finite.
__host__ __device__ __forceinline__ bool rs_p3p_pose(const RsP3P &q, double v, RsPose &o) {
    const double den = 2.0 * (q.cg - v * q.ca);
    const double u = ((((q.p - 1.0) * (v * v) - 2.0 * q.p * q.cb * v) + 1.0) + q.p) / den;
    const double s1 = sqrt(q.b2 / ((1.0 + v * v) - 2.0 * v * q.cb)), s2 = u * s1, s3 = v * s1;
    double Y[3][3], FX[3][3], FY[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Y[0][i] = s1 * q.f[0][i];
        Y[1][i] = s2 * q.f[1][i];
        Y[2][i] = s3 * q.f[2][i];
    }
    rs_frame(q.X[0], q.X[1], q.X[2], FX);
    rs_frame(Y[0], Y[1], Y[2], FY);
    bool ok = v > 0.0 && den != 0.0 && u > 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o.R[3 * r + c] = FY[r][0] * FX[c][0] + FY[r][1] * FX[c][1] + FY[r][2] * FX[c][2];
            ok = ok && pose_finite(o.R[3 * r + c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o.t[r] = Y[0][r] - (o.R[3 * r] * q.X[0][0] + o.R[3 * r + 1] * q.X[0][1] + o.R[3 * r + 2] * q.X[0][2]);
        ok = ok && pose_finite(o.t[r]);
    }
    return ok;
}

// Candidate c = 4 k + j of a sample: root j, in ascending order, of the sample's quartic.  False if the sample is invalid,
// it has no root j or that root's pose is skipped.
__host__ __device__ __forceinline__ bool rs_candidate_pose(const RsCorr (&s)[3], const float *K, unsigned j, RsPose &o) {
    RsP3P q;
    if (!rs_p3p_quartic(s, K, q)) return false;
    double r[4];
    const unsigned n = (unsigned)rs_real_roots<4>(q.A, q.B, r);
    const double v = j == 0 ? r[0] : j == 1 ? r[1] : j == 2 ? r[2] : r[3];
    const bool ok = rs_p3p_pose(q, v, o);
    return ok && j < n;
}

// Step 4 for an f64 pose, tri_error2's operations: p = R X + t (each row summed left to right); false if not in front.
// (K is float as the arrays hold it, or double for bundle adjustment's refined intrinsics: double(K[i]) is then the identity,
// and a widened f32 value gives the same bits either way)
template <typename T, typename KT>
__host__ __device__ __forceinline__ bool rs_error2(const RsPose &P, const KT *K, const RsCorrT<T> &c, double &e2) {
    double p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = P.R[3 * r] * double(c.X) + P.R[3 * r + 1] * double(c.Y) + P.R[3 * r + 2] * double(c.Z) + P.t[r];
    const double ex = double(K[0]) * (p[0] / p[2]) + double(K[2]) - double(c.x);
    const double ey = double(K[1]) * (p[1] / p[2]) + double(K[3]) - double(c.y);
    e2 = ex * ex + ey * ey;
    return p[2] > 0.0;
}
template <typename T, typename KT>
__host__ __device__ __forceinline__ bool rs_inlier(const RsPose &P, const KT *K, const RsCorrT<T> &c, double thr2, double &e2) {
    const bool front = rs_error2(P, K, c, e2);
    return front && e2 <= thr2;
}
// the MSAC term of a correspondence: min(e^2, thr2), thr2 for a point not in front (or a NaN)
template <typename T, typename KT>
__host__ __device__ __forceinline__ double rs_cost(const RsPose &P, const KT *K, const RsCorrT<T> &c, double thr2) {
    double e2;
    return rs_inlier(P, K, c, thr2, e2) ? e2 : thr2;
}

// Step 5: the 27 values an inlier adds to the normal equations of the step (w, dt), R' = C(w) R, t' = t + dt.  With q = R X,
// p = q + t, a = fx / p_z, b = fy / p_z: d e_x / d p = (a, 0, -a p_x / p_z), d e_y / d p = (0, b, -b p_y / p_z), d p / d w =
// -2 [q]x (C(w) = I + 2 [w]x + O(w^2)), d p / d dt = I.
// The rows themselves (bundle adjustment, mkd_bundle_math.h, needs them beside the point's): Jx, Jy, the residual and the
// factors a, b, gx, gy of d e / d p, and the normalised projection (u, v) = (p_x / p_z, p_y / p_z) the residual was formed from.
struct RsRows {
    double Jx[6], Jy[6], ex, ey, a, b, gx, gy, u, v;
};
template <typename T, typename KT>
__host__ __device__ __forceinline__ void rs_gn_rows(const RsPose &P, const KT *K, const RsCorrT<T> &c, RsRows &o) {
    double q[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        q[r] = P.R[3 * r] * double(c.X) + P.R[3 * r + 1] * double(c.Y) + P.R[3 * r + 2] * double(c.Z);
        p[r] = q[r] + P.t[r];
    }
    const double px = p[0] / p[2], py = p[1] / p[2];
    o.ex = double(K[0]) * px + double(K[2]) - double(c.x);
    o.ey = double(K[1]) * py + double(K[3]) - double(c.y);
    const double a = double(K[0]) / p[2], b = double(K[1]) / p[2];
    const double gx = 0.0 - a * px, gy = 0.0 - b * py;
    const double Jx[6] = {2.0 * (gx * q[1]), 2.0 * (a * q[2] - gx * q[0]), 2.0 * (0.0 - a * q[1]), a, 0.0, gx};
    const double Jy[6] = {2.0 * (gy * q[1] - b * q[2]), 2.0 * (0.0 - gy * q[0]), 2.0 * (b * q[0]), 0.0, b, gy};
#pragma unroll
    for (int i = 0; i < 6; ++i) o.Jx[i] = Jx[i], o.Jy[i] = Jy[i];
    o.a = a, o.b = b, o.gx = gx, o.gy = gy, o.u = px, o.v = py;
}
// the 27 values of two rows and their residual: J^T J's upper triangle row by row, then J^T e
__host__ __device__ __forceinline__ void rs_gn_products(const RsRows &r, double *w) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) w[n++] = r.Jx[i] * r.Jx[j] + r.Jy[i] * r.Jy[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[21 + i] = r.Jx[i] * r.ex + r.Jy[i] * r.ey;
}
template <typename T, typename KT>
__host__ __device__ __forceinline__ void rs_gn_terms(const RsPose &P, const KT *K, const RsCorrT<T> &c, double *w) {
    RsRows r;
    rs_gn_rows(P, K, c, r);
    rs_gn_products(r, w);
}

// Solves H d = g for the symmetric 6x6 H of the 27 sums by Cholesky (d returned in x); false at the first pivot that is not
// positive (a NaN included).  Every loop has constant bounds: the matrix stays in registers.
__host__ __device__ __forceinline__ bool rs_cholesky6(const double *w, double (&x)[6]) {
    double N[6][6];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) N[i][j] = w[n++];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = w[21 + i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = N[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - N[k][j] * N[k][j];
        ok = ok && d > 0.0;
        const double l = sqrt(d);
        N[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = N[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - N[k][j] * N[k][i];
            N[j][i] = s / l;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - N[k][i] * x[k];
        x[i] = s / N[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - N[i][k] * x[k];
        x[i] = s / N[i][i];
    }
    return ok;
}

// Step 5's update from the solution d of H d = J^T e: w = 0 - d[0 .. 2], dt = 0 - d[3 .. 5], R' = C(w) R with the Cayley map
// C(w) = ((1 - w.w) I + 2 w w^T + 2 [w]x) / (1 + w.w), t' = t + dt.
__host__ __device__ __forceinline__ void rs_update(const RsPose &P, const double (&d)[6], RsPose &o) {
    const double w0 = 0.0 - d[0], w1 = 0.0 - d[1], w2 = 0.0 - d[2];
    const double n = w0 * w0 + w1 * w1 + w2 * w2, k = 1.0 - n, s = 1.0 + n;
    const double C[9] = {(k + 2.0 * (w0 * w0)) / s,       (2.0 * (w0 * w1) - 2.0 * w2) / s, (2.0 * (w0 * w2) + 2.0 * w1) / s,
                         (2.0 * (w0 * w1) + 2.0 * w2) / s, (k + 2.0 * (w1 * w1)) / s,       (2.0 * (w1 * w2) - 2.0 * w0) / s,
                         (2.0 * (w0 * w2) - 2.0 * w1) / s, (2.0 * (w1 * w2) + 2.0 * w0) / s, (k + 2.0 * (w2 * w2)) / s};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = C[3 * r] * P.R[c] + C[3 * r + 1] * P.R[3 + c] + C[3 * r + 2] * P.R[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) o.t[r] = P.t[r] - d[3 + r];
}

// Step 6's combine of the 256 slot sums of ONE value: within each run of 64 slots the butterfly over slot xor 32, 16, .. 1,
// then ((w0 + w1) + w2) + w3.  (Addition commutes bit for bit, so every lane of a wave ends with lane 0's value.)  Changes s.
__host__ __device__ __forceinline__ double rs_combine(double *s) {
    for (int m = 32; m >= 1; m >>= 1)
        for (int j = 0; j < kRsSlots; ++j)
            if (!(j & m)) {
                const double v = s[j] + s[j ^ m];
                s[j] = v;
                s[j ^ m] = v;
            }
    return ((s[0] + s[64]) + s[128]) + s[192];
}

// Step 7: the f64 pose rounded to f32 into an observation record for tri_inlier
__host__ __device__ __forceinline__ void rs_round(const RsPose &P, const float *K, TriObs &o) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o.K[i] = K[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) o.P[i] = float(P.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.P[9 + i] = float(P.t[i]);
}

}  // namespace
}  // namespace lfmkd
