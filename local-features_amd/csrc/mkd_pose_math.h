// The arithmetic of the two-view pose call (mkd_two_view_pose.hip; algorithm: include/lf_mkd.h, lf_mkd_two_view_pose_device):
// the essential matrix, its SVD through a fixed-sweep Jacobi of E^T E, the four (R, t) candidates, a link's in-front test and
// its triangulated point, every one __host__ __device__.  tests/cpp/pose_twin.cpp includes it under a plain C++ compiler
// (with -ffp-contract=off) and restates only the kernel's orchestration, so the host twin the device is held to bit for bit
// (tests/test_gpu_two_view_pose.py) is this code and no transcription of it.  Needs <math.h> and <stdint.h> alone.
// Everything is a fixed sequence of correctly rounded f64 operations (+ - * /, sqrt) under contraction OFF.  The Jacobi is
// mkd_fundamental_math.h's smallest_eigenvector restated (that one keeps one column only, and the verifier's bits stay as
// they are).  As there, no product is negated by a unary minus (clang does not apply the contraction pragma to it): signs
// go onto a value that exists already, and a difference of products is written as a difference.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_verify_pair.h"   // the HIP qualifiers defined away without hipcc

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr int kPoseSweeps = 6;          // cyclic Jacobi sweeps (the F refit's count)
constexpr double kPoseRank = 1e-3;      // s2 at or below this times s1: E has no second direction, no pose
constexpr unsigned kPoseNone = 0xFFFFFFFFu;

// What step 2 leaves of an edge: the two twisted rotations (row-major), u3 (t = +u3 for candidates 0 and 2, -u3 for 1 and 3)
// and the singular values over the largest.
struct PoseFrame {
    double R[2][9], u3[3], sigma[3];
};

__host__ __device__ __forceinline__ bool pose_finite(double v) { return v - v == 0.0; }
// max(v, 0) as a select: +0 for -0, a negative value and a NaN, on every compiler
__host__ __device__ __forceinline__ double pose_floor0(double v) { return v > 0.0 ? v : 0.0; }

// Step 1: E = Kb^T F Ka in f64 (K = fx, fy, cx, cy).  False if an intrinsic is not finite, fx or fy is not positive, a value
// of F is not finite, or F is all zero.
__host__ __device__ __forceinline__ bool pose_essential(const float *F, const float *Ka, const float *Kb, double (&E)[9]) {
    bool ok = true, any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) ok = ok && pose_finite(double(Ka[i])) && pose_finite(double(Kb[i]));
    ok = ok && Ka[0] > 0.f && Ka[1] > 0.f && Kb[0] > 0.f && Kb[1] > 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        ok = ok && pose_finite(double(F[i]));
        any = any || F[i] != 0.f;
    }
    const double fxa = Ka[0], fya = Ka[1], cxa = Ka[2], cya = Ka[3], fxb = Kb[0], fyb = Kb[1], cxb = Kb[2], cyb = Kb[3];
    double M[9];   // F Ka
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double f0 = F[3 * r], f1 = F[3 * r + 1], f2 = F[3 * r + 2];
        M[3 * r] = f0 * fxa;
        M[3 * r + 1] = f1 * fya;
        M[3 * r + 2] = f0 * cxa + f1 * cya + f2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        E[c] = fxb * M[c];
        E[3 + c] = fyb * M[3 + c];
        E[6 + c] = cxb * M[c] + cyb * M[3 + c] + M[6 + c];
    }
    return ok && any;
}

// Cyclic Jacobi on the symmetric 3x3 S (pairs (0,1) (0,2) (1,2), kPoseSweeps sweeps, the textbook rotation:
// theta = (s_qq - s_pp) / (2 s_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), none where s_pq = 0): S's diagonal
// becomes the eigenvalues, V's columns the eigenvectors.
__host__ __device__ __forceinline__ void pose_jacobi(double (&S)[3][3], double (&V)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kPoseSweeps; ++sweep) {
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
}

__host__ __device__ __forceinline__ double pose_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ __forceinline__ void pose_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// y = E x, E row-major
__host__ __device__ __forceinline__ void pose_apply(const double *E, const double *x, double *y) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = E[3 * r] * x[0] + E[3 * r + 1] * x[1] + E[3 * r + 2] * x[2];
}

// Step 2: false (no pose) if s1 is not finite and positive or s2 <= kPoseRank s1.
__host__ __device__ __forceinline__ bool pose_decompose(const double (&E)[9], PoseFrame &P) {
    double S[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
    pose_jacobi(S, V);
    // descending, the lower index first on a tie: i1 the first of the largest, i3 the last of the smallest, i2 the one left
    // (i1 != i3 whatever the values are, a NaN included: every comparison with it is false)
    const double w0 = S[0][0], w1 = S[1][1], w2 = S[2][2];
    const int i1 = w1 > w0 ? (w2 > w1 ? 2 : 1) : (w2 > w0 ? 2 : 0);
    const int i3 = w2 <= w1 ? (w0 < w2 ? 0 : 2) : (w0 < w1 ? 0 : 1);
    const int i2 = 3 - i1 - i3;
    double s[3], v1[3], v2[3], v3[3];
    s[0] = sqrt(pose_floor0(i1 == 0 ? w0 : i1 == 1 ? w1 : w2));
    s[1] = sqrt(pose_floor0(i2 == 0 ? w0 : i2 == 1 ? w1 : w2));
    s[2] = sqrt(pose_floor0(i3 == 0 ? w0 : i3 == 1 ? w1 : w2));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v1[k] = i1 == 0 ? V[k][0] : i1 == 1 ? V[k][1] : V[k][2];
        v2[k] = i2 == 0 ? V[k][0] : i2 == 1 ? V[k][1] : V[k][2];
    }
    const bool ok = pose_finite(s[0]) && s[0] > 0.0 && s[1] > kPoseRank * s[0];
    double u1[3], u2[3], u3[3], e1[3], e2[3];
    pose_apply(E, v1, e1);
    const double n1 = sqrt(pose_dot(e1, e1));
#pragma unroll
    for (int k = 0; k < 3; ++k) u1[k] = e1[k] / n1;
    pose_apply(E, v2, e2);
    const double along = pose_dot(u1, e2);
#pragma unroll
    for (int k = 0; k < 3; ++k) e2[k] = e2[k] - along * u1[k];
    const double n2 = sqrt(pose_dot(e2, e2));
#pragma unroll
    for (int k = 0; k < 3; ++k) u2[k] = e2[k] / n2;
    pose_cross(u1, u2, u3);
    pose_cross(v1, v2, v3);
    // R1 = U W V^T = u2 v1^T - u1 v2^T + u3 v3^T, R2 = U W^T V^T = u1 v2^T - u2 v1^T + u3 v3^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double a = u2[i] * v1[j], b = u1[i] * v2[j], c = u3[i] * v3[j];
            P.R[0][3 * i + j] = (a - b) + c;
            P.R[1][3 * i + j] = (b - a) + c;
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) P.u3[k] = u3[k];
    P.sigma[0] = 1.0;
    P.sigma[1] = s[1] / s[0];
    P.sigma[2] = s[2] / s[0];
    return ok;
}

// a keypoint's ray: ((x - cx) / fx, (y - cy) / fy, 1)
__host__ __device__ __forceinline__ void pose_ray(float x, float y, const float *K, double *r) {
    r[0] = (double(x) - double(K[2])) / double(K[0]);
    r[1] = (double(y) - double(K[3])) / double(K[1]);
    r[2] = 1.0;
}

// Step 3 for one link under (R, t): p = R xa, q = xb.
struct PoseLink {
    double pp, qq, pq, det, na, nb;
};
__host__ __device__ __forceinline__ PoseLink pose_link(const double *R, const double *t, const double *xa, const double *xb) {
    double p[3];
    pose_apply(R, xa, p);
    PoseLink L;
    L.pp = pose_dot(p, p);
    L.qq = pose_dot(xb, xb);
    L.pq = pose_dot(p, xb);
    const double pt = pose_dot(p, t), qt = pose_dot(xb, t);
    L.det = L.pp * L.qq - L.pq * L.pq;
    L.na = L.pq * qt - pt * L.qq;
    L.nb = L.pp * qt - L.pq * pt;
    return L;
}
__host__ __device__ __forceinline__ bool pose_front(const PoseLink &L) { return L.det > 0.0 && L.na > 0.0 && L.nb > 0.0; }
// (of a link that is in front)
__host__ __device__ __forceinline__ bool pose_parallax(const PoseLink &L, double cmin) { return L.pq <= cmin * sqrt(L.pp * L.qq); }

// the translation of candidate c: +u3 for 0 and 2, -u3 for 1 and 3 (the sign of a value, exact)
__host__ __device__ __forceinline__ void pose_translation(const PoseFrame &P, unsigned c, double *t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (c & 1u) ? -P.u3[k] : P.u3[k];
}

// The four candidates' in-front tests of one link, as bits 0..3.
__host__ __device__ __forceinline__ unsigned pose_votes(const PoseFrame &P, const double *xa, const double *xb) {
    unsigned bits = 0;
#pragma unroll
    for (unsigned c = 0; c < 4; ++c) {
        double t[3];
        pose_translation(P, c, t);
        bits |= pose_front(pose_link(P.R[c >> 1], t, xa, xb)) ? 1u << c : 0u;
    }
    return bits;
}

// Step 4: the largest count (`best`), the lowest c on a tie; kPoseNone if it is 0.  `other` = the largest of the other three.
__host__ __device__ __forceinline__ unsigned pose_choose(const unsigned *count, unsigned &best, unsigned &other) {
    unsigned c = 0;
    best = count[0];
#pragma unroll
    for (unsigned k = 1; k < 4; ++k) {
        const bool take = count[k] > best;
        c = take ? k : c;
        best = take ? count[k] : best;
    }
    other = 0;
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) other = k != c && count[k] > other ? count[k] : other;
    return best ? c : kPoseNone;
}

// Step 5: X = (la xa + R^T (lb xb - t)) / 2 and the cosine of the parallax angle, rounded to f32, of a link that is in front.
__host__ __device__ __forceinline__ void pose_point(const double *R, const double *t, const double *xa, const double *xb,
                                                    const PoseLink &L, float *out) {
    const double la = L.na / L.det, lb = L.nb / L.det;
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = lb * xb[k] - t[k];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double r = R[j] * w[0] + R[3 + j] * w[1] + R[6 + j] * w[2];
        out[j] = float(0.5 * (la * xa[j] + r));
    }
    out[3] = float(L.pq / sqrt(L.pp * L.qq));
}

}  // namespace
}  // namespace lfmkd
