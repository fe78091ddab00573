// gfx950 two-view poses (include/lf_mkd.h, lf_mkd_two_view_pose_device): per edge of a link table the relative
// pose (R, t) its fundamental matrix gives under the two images' intrinsics, chosen among the four candidates by a vote of the
// edge's links, and the links' triangulated points.  The arithmetic is csrc/mkd_pose_math.h, which the host twin compiles too.
//
//   two_view_pose   ONE launch, one workgroup of 256 threads per edge.  Thread 0 forms E and its decomposition (a serial
//                   chain of f64 operations: a few thousand instructions, once per edge) and leaves the frame in LDS; the
//                   workgroup then walks the edge's links 256 at a time and counts the four candidates' in-front links (a
//                   ballot and a popcount per wave, the four waves' counts summed in LDS: integer sums, no order in them),
//                   every thread makes the same choice from the same four counts, and a second walk writes the points and
//                   counts the links with parallax under the chosen pose.
//
// No scratch memory, no allocation, no atomic, and no workgroup waits for another; both walks are wave-uniform (a wave whose
// lanes have no link left goes through the step with its predicate off), so the ballots see whole waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_pose_math.h"
#include "mkd_scene.h"   // clamp_to

namespace lfmkd {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

// link k of the table: false if a row is outside the pool; else the two rays
__device__ __forceinline__ bool load_link(const float *__restrict__ kps, uint64_t n_rows, const int *__restrict__ link_a,
                                          const int *__restrict__ link_b, uint64_t k, const float *Ka, const float *Kb,
                                          double *xa, double *xb) {
    const int ra = link_a[k], rb = link_b[k];
    if (ra < 0 || rb < 0 || (uint64_t)ra >= n_rows || (uint64_t)rb >= n_rows) return false;
    pose_ray(kps[5 * (uint64_t)ra], kps[5 * (uint64_t)ra + 1], Ka, xa);
    pose_ray(kps[5 * (uint64_t)rb], kps[5 * (uint64_t)rb + 1], Kb, xb);
    return true;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void two_view_pose(const float *__restrict__ kps, uint64_t n_rows,
                                                          const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                          const float *__restrict__ intrinsics, unsigned n_images,
                                                          const float *__restrict__ F, const uint64_t *__restrict__ link_off,
                                                          const int *__restrict__ link_a, const int *__restrict__ link_b,
                                                          uint64_t link_capacity, double cmin, float *__restrict__ R_out,
                                                          float *__restrict__ t_out, unsigned *__restrict__ stats,
                                                          float *__restrict__ sigma, float *__restrict__ points) {
    __shared__ PoseFrame s_frame;
    __shared__ float s_K[8];
    __shared__ unsigned s_ok, s_cnt[kWaves][4];
    const unsigned e = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t lo = clamp_to(link_off[e], link_capacity), hi_raw = clamp_to(link_off[e + 1], link_capacity);
    const uint64_t hi = hi_raw > lo ? hi_raw : lo;
    if (tid == 0) {
        const unsigned a = edge_a[e], b = edge_b[e];
        bool ok = a < n_images && b < n_images;
        if (ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s_K[i] = intrinsics[4 * (uint64_t)a + i];
                s_K[4 + i] = intrinsics[4 * (uint64_t)b + i];
            }
            double E[9];
            ok = pose_essential(F + 9 * (uint64_t)e, s_K, s_K + 4, E);
            PoseFrame P;
            ok = pose_decompose(E, P) && ok;
            s_frame = P;
        }
        s_ok = ok;
    }
    __syncthreads();
    const bool have = s_ok != 0;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    if (have) {                                                                   // workgroup-uniform
        for (uint64_t k0 = lo + 64 * wave; k0 < hi; k0 += kThreads) {             // wave-uniform
            const uint64_t k = k0 + lane;
            double xa[3], xb[3];
            unsigned bits = 0;
            if (k < hi && load_link(kps, n_rows, link_a, link_b, k, s_K, s_K + 4, xa, xb)) bits = pose_votes(s_frame, xa, xb);
#pragma unroll
            for (int c = 0; c < 4; ++c) cnt[c] += (unsigned)__popcll(__ballot((bits >> c) & 1u));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) cnt[c] = s_cnt[0][c] + s_cnt[1][c] + s_cnt[2][c] + s_cnt[3][c];
    unsigned best = 0, other = 0;
    const unsigned c = have ? pose_choose(cnt, best, other) : kPoseNone;
    const bool pose = c != kPoseNone;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (c & 2u) ? s_frame.R[1][i] : s_frame.R[0][i];
    pose_translation(s_frame, c, t);
    __syncthreads();                                                              // s_cnt is read; the second walk reuses it
    unsigned par = 0;
    if (pose || points) {
        for (uint64_t k0 = lo + 64 * wave; k0 < hi; k0 += kThreads) {
            const uint64_t k = k0 + lane;
            double xa[3], xb[3];
            float out[4] = {0.f, 0.f, 0.f, 2.f};
            bool wide = false;
            if (pose && k < hi && load_link(kps, n_rows, link_a, link_b, k, s_K, s_K + 4, xa, xb)) {
                const PoseLink L = pose_link(R, t, xa, xb);
                if (pose_front(L)) {
                    wide = pose_parallax(L, cmin);
                    pose_point(R, t, xa, xb, L, out);
                }
            }
            par += (unsigned)__popcll(__ballot(wide));
            if (points && k < hi) {                                               // (d_points is only 4-byte aligned)
#pragma unroll
                for (int i = 0; i < 4; ++i) points[4 * k + i] = out[i];
            }
        }
    }
    if (lane == 0) s_cnt[wave][0] = par;
    __syncthreads();
    if (tid < 9) R_out[9 * (uint64_t)e + tid] = pose ? float(s_frame.R[(c >> 1) & 1u][tid]) : 0.f;
    if (tid < 3) {
        t_out[3 * (uint64_t)e + tid] = pose ? float((c & 1u) ? -s_frame.u3[tid] : s_frame.u3[tid]) : 0.f;
        if (sigma) sigma[3 * (uint64_t)e + tid] = pose ? float(s_frame.sigma[tid]) : 0.f;
    }
    if (tid == 0) {
        unsigned *st = stats + 4 * (uint64_t)e;
        st[0] = pose ? best : 0u;
        st[1] = pose ? other : 0u;
        st[2] = c;
        st[3] = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    }
}

void launch_two_view_pose(const float *kps, uint64_t n_rows, const unsigned *edge_a, const unsigned *edge_b, unsigned n_edges,
                          const float *intrinsics, unsigned n_images, const float *F, const uint64_t *link_off, const int *link_a,
                          const int *link_b, uint64_t link_capacity, double cmin, float *R, float *t, unsigned *stats, float *sigma,
                          float *points, hipStream_t stream) {
    if (n_edges == 0) return;
    hipLaunchKernelGGL(two_view_pose, dim3(n_edges), dim3(kThreads), 0, stream, kps, n_rows, edge_a, edge_b, intrinsics, n_images,
                       F, link_off, link_a, link_b, link_capacity, cmin, R, t, stats, sigma, points);
}

}  // namespace lfmkd
