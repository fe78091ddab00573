// The arithmetic of the view-graph call (mkd_view_graph.hip; algorithm: include/lf_mkd.h, lf_mkd_view_graph_device): the
// usable test, the quaternion of a rotation matrix, the product and the conjugate, the loop test, an edge's state, the tree's
// edge ordering, the prediction's sign, the averaging step over the 4-slot canonical sum, the rotation of a quaternion and the
// residual cosine, every one __host__ __device__.  tests/cpp/view_graph_twin.cpp includes it under a plain C++ compiler (with
// -ffp-contract=off) and restates only the kernels' orchestration, so the host twin the device is held to bit for bit
// (tests/test_gpu_view_graph.py) is this code and no transcription of it.  Needs <math.h> and <stdint.h> alone.  Everything is
// a fixed sequence of correctly rounded f64 operations (+ - * /, sqrt) under contraction OFF; as in mkd_pose_math.h no value is
// negated by a unary minus: "0 - x" is written as a difference.  A quaternion is (w, x, y, z), the product is Hamilton's, and
// the rotation of q1 (x) q2 is the rotation of q1 times that of q2.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_triangulate_math.h"   // tri_combine, the 4-slot canonical sum; pose_finite through it

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr unsigned kVgNone = 0xFFFFFFFFu;
constexpr int kVgSlots = 4;                 // the averaging's sum is mkd_triangulate_math.h's 4-slot one
static_assert(kTriSlots == kVgSlots, "the view graph's averaging is specified over tri_combine's 4 slots");
enum : unsigned { kVgUnusable = 0, kVgRejected = 1, kVgUnchecked = 2, kVgSupported = 3 };

struct VgQuat {
    double w, x, y, z;
};

// Definition 1: both ids in range and different, a pose (stats[2] != none) with at least min_front links in front, nine
// finite entries.
__host__ __device__ __forceinline__ bool vg_usable(unsigned a, unsigned b, unsigned n_images, const unsigned *stats, const float *R,
                                                   unsigned min_front) {
    bool ok = a < n_images && b < n_images && a != b && stats[2] != kVgNone && stats[0] >= min_front;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && pose_finite(double(R[i]));
    return ok;
}

__host__ __device__ __forceinline__ VgQuat vg_normalise(const VgQuat &q) {
    const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    return VgQuat{q.w / n, q.x / n, q.y / n, q.z / n};
}

// Definition 2, Shepperd's method: the largest of (trace, R00, R11, R22), the lowest index on a tie, picks which component is
// formed from the diagonal (u = 1 + 2 max - trace >= 1, so the norm is never 0); the other three come from the off-diagonal
// sums and differences; one normalisation.  (The four unnormalised forms are 4 q_k q for k = w, x, y, z.)
__host__ __device__ __forceinline__ VgQuat vg_from_rotation(const float *Rf) {
    const double r00 = double(Rf[0]), r01 = double(Rf[1]), r02 = double(Rf[2]), r10 = double(Rf[3]), r11 = double(Rf[4]),
                 r12 = double(Rf[5]), r20 = double(Rf[6]), r21 = double(Rf[7]), r22 = double(Rf[8]);
    const double t = r00 + r11 + r22;
    int k = 0;
    double best = t;
    if (r00 > best) k = 1, best = r00;
    if (r11 > best) k = 2, best = r11;
    if (r22 > best) k = 3, best = r22;
    VgQuat q;
    if (k == 0) q = VgQuat{1.0 + r00 + r11 + r22, r21 - r12, r02 - r20, r10 - r01};
    else if (k == 1) q = VgQuat{r21 - r12, 1.0 + r00 - r11 - r22, r01 + r10, r02 + r20};
    else if (k == 2) q = VgQuat{r02 - r20, r01 + r10, 1.0 - r00 + r11 - r22, r12 + r21};
    else q = VgQuat{r10 - r01, r02 + r20, r12 + r21, 1.0 - r00 - r11 + r22};
    return vg_normalise(q);
}

__host__ __device__ __forceinline__ VgQuat vg_mul(const VgQuat &a, const VgQuat &b) {
    return VgQuat{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                  a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
// Definition 3: a representative's quaternion in the direction asked for -- conjugated iff it is stored the other way round
__host__ __device__ __forceinline__ VgQuat vg_directed(const VgQuat &q, bool reversed) {
    return reversed ? VgQuat{q.w, 0.0 - q.x, 0.0 - q.y, 0.0 - q.z} : q;
}
__host__ __device__ __forceinline__ double vg_dot(const VgQuat &a, const VgQuat &b) {
    return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;
}

// Definition 4: L = q(c->a) (x) (q(b->c) (x) q_e) closes the loop iff the cosine of its angle, 2 L_w^2 - 1, is at least cmax
__host__ __device__ __forceinline__ bool vg_loop_closes(const VgQuat &q_ca, const VgQuat &q_bc, const VgQuat &q_e, double cmax) {
    const VgQuat L = vg_mul(q_ca, vg_mul(q_bc, q_e));
    return 2.0 * (L.w * L.w) - 1.0 >= cmax;
}
// Definition 5, of a usable edge
__host__ __device__ __forceinline__ unsigned vg_state(unsigned closed, unsigned consistent) {
    return consistent ? kVgSupported : closed ? kVgRejected : kVgUnchecked;
}
// Definition 6
__host__ __device__ __forceinline__ bool vg_kept_state(unsigned state, bool use_unchecked) {
    return state == kVgSupported || (use_unchecked && state == kVgUnchecked);
}

// Definition 8's order of the kept edges an image may take, as one key: the larger key wins.  State first (a kept edge is
// supported or unchecked: one bit), then the links in front, then the LOWER edge index (below 2^31 - 1, so the last field is
// at least 1 and 0 is "no edge").
__host__ __device__ __forceinline__ uint64_t vg_tree_key(unsigned state, unsigned front, unsigned edge) {
    return (uint64_t(state == kVgSupported) << 63) | (uint64_t(front) << 31) | uint64_t(0x7FFFFFFFu - edge);
}
__host__ __device__ __forceinline__ unsigned vg_tree_key_edge(uint64_t key) { return 0x7FFFFFFFu - unsigned(key & 0x7FFFFFFFu); }

// Definitions 8 and 9: image i's value as its neighbour j predicts it over their pair's representative
__host__ __device__ __forceinline__ VgQuat vg_predict(const VgQuat &q_ji, const VgQuat &q_j) { return vg_mul(q_ji, q_j); }
// ... on q_i's side of the sphere
__host__ __device__ __forceinline__ VgQuat vg_towards(const VgQuat &p, const VgQuat &q_i) {
    return vg_dot(p, q_i) < 0.0 ? VgQuat{0.0 - p.w, 0.0 - p.x, 0.0 - p.y, 0.0 - p.z} : p;
}
// Definition 9's step: slot[s] holds, per component, the sum of the terms k = s, s + 4, .. in ascending k (k counts the terms
// in ascending order of the neighbour's id); the four slots are combined by tri_combine, the lazy term n q_i is added, and
// the result is normalised.  n == 0: q_i as it is.
__host__ __device__ __forceinline__ VgQuat vg_average(const VgQuat *slot, unsigned n, const VgQuat &q_i) {
    if (n == 0) return q_i;
    const double w[4] = {slot[0].w, slot[1].w, slot[2].w, slot[3].w}, x[4] = {slot[0].x, slot[1].x, slot[2].x, slot[3].x};
    const double y[4] = {slot[0].y, slot[1].y, slot[2].y, slot[3].y}, z[4] = {slot[0].z, slot[1].z, slot[2].z, slot[3].z};
    const double m = double(n);
    return vg_normalise(VgQuat{tri_combine(w) + m * q_i.w, tri_combine(x) + m * q_i.x, tri_combine(y) + m * q_i.y,
                               tri_combine(z) + m * q_i.z});
}

// Definition 10: the rotation of a unit quaternion, row-major, rounded to f32
__host__ __device__ __forceinline__ void vg_rotation(const VgQuat &q, float *R) {
    const double ww = q.w * q.w, xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z;
    const double xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z, wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
    R[0] = float(ww + xx - yy - zz);
    R[1] = float(2.0 * (xy - wz));
    R[2] = float(2.0 * (xz + wy));
    R[3] = float(2.0 * (xy + wz));
    R[4] = float(ww - xx + yy - zz);
    R[5] = float(2.0 * (yz - wx));
    R[6] = float(2.0 * (xz - wy));
    R[7] = float(2.0 * (yz + wx));
    R[8] = float(ww - xx - yy + zz);
}
// ... and an edge's residual: the cosine of the angle between R and R_b R_a^T
__host__ __device__ __forceinline__ float vg_residual(const VgQuat &q_b, const VgQuat &q_e, const VgQuat &q_a) {
    const double d = vg_dot(q_b, vg_mul(q_e, q_a));
    return float(2.0 * (d * d) - 1.0);
}

}  // namespace
}  // namespace lfmkd
