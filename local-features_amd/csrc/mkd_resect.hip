// gfx950 camera resection (include/lf_mkd.h, lf_mkd_resect_cameras_device): the absolute pose [R | t] of an
// image from the 2-D keypoints it owns in tracks that have a 3-D point -- P3P samples scored by reprojection inliers, a
// Gauss-Newton refit over the winner's inliers, the f32 rounding and the final inliers.  The arithmetic is
// csrc/mkd_resect_math.h, which the host twin compiles too.  Three launches, every one sized on the host from the call's
// arguments alone; the scalars (T, the image ranges, M) are read on the device.
//
//   rs_gather   a workgroup per image.  It decides CANDIDACY from d_poses and writes it, with M, into scratch: rs_select, the
//               only kernel that stores to d_poses_out, reads that flag and never d_poses' R again to decide, so the call may
//               run in place.  A candidate's rows are walked 256 at a time and the correspondences compacted in ascending
//               order (ballot, popcount, the waves' counts through LDS, a running base: no atomic decides a position) into
//               scratch at the image's own row range, 4 bytes a row, so no scan across images is needed.  It zeroes the
//               image's candidate counts and writes d_row_state's 0 / 1.
//   rs_score    the hot path.  Grid: image x block of 256 candidates x slice of positions.  A lane owns ONE candidate c
//               (sample c / 4, root c % 4): the four lanes of a sample solve the same quartic and each keeps 12 f64.  The
//               correspondences are staged 256 at a time in LDS as {x, y, X, Y, Z} and read as broadcasts.  A slice is every
//               (slices)-th run of kRsSliceLen positions; a slice beyond M ends before it solves anything.  A valid
//               candidate's count goes to scratch [image][4 n_samples] by integer atomic add, plus 1 from slice 0, so that 0
//               says "no candidate" and the sum is exact whatever the order.
//   rs_select   a workgroup per image: argmax over (count, lowest c), the winner's pose again by the same code, the refit
//               rounds as block passes (thread s IS slot s of the canonical sum), the rounding, the final pass, the outputs.
//
// Scratch belongs to the handle (lf_mkd.cpp); no allocation here, nobody waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_resect_math.h"
#include "mkd_scene.h"

namespace lfmkd {
namespace {

constexpr int kThreads = kRsSlots;
constexpr int kWaves = kThreads / 64;
static_assert(kThreads == kSumThreads, "thread s is slot s of the canonical sum");
constexpr unsigned kRsSliceLen = 1024;      // positions of a run of rs_score: 4 LDS stages
constexpr unsigned kRsMaxSlices = 16;       // slices a launch has at most; slice z takes the runs z, z + slices, ..

// scratch: idx [n_rows] (image i's correspondences' rows at [lo_i, lo_i + M_i)), head [n_images][2] = {M, candidate},
// votes [n_images][4 n_samples]
struct RsScratch {
    unsigned *idx, *head, *votes;
};

// the correspondence a compacted position names (its row passed rs_gather's test, so the indices are in range)
__device__ __forceinline__ RsCorr load_corr(const SceneTables &in, const float *points, unsigned row) {
    const float *k = in.kps + 5 * (uint64_t)row, *p = points + 4 * (uint64_t)in.row_track[row];
    return RsCorr{k[0], k[1], p[0], p[1], p[2]};
}

}  // namespace

__global__ __launch_bounds__(kThreads) void rs_gather(SceneTables in, const float *points, const float *__restrict__ poses,
                                                      unsigned n_samples, double cmin, unsigned all, RsScratch sc,
                                                      unsigned *__restrict__ row_state) {
    __shared__ unsigned s_cnt[kWaves];
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    float K[4], P[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = poses[12 * (uint64_t)img + i];
    const bool cand = rs_candidate(K, P, all != 0);
    if (!cand) {                                                             // block-uniform
        if (tid == 0) sc.head[2 * (uint64_t)img] = 0, sc.head[2 * (uint64_t)img + 1] = 0;
        return;
    }
    for (unsigned c = tid; c < 4 * n_samples; c += kThreads) sc.votes[(uint64_t)img * 4 * n_samples + c] = 0;
    const uint64_t T = clamp_to(in.counts[0], in.tcap);
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    uint64_t base = lo;
    for (uint64_t r0 = lo; r0 < hi; r0 += kThreads) {                        // block-uniform
        const uint64_t r = r0 + tid;
        bool is = false;
        if (r < hi) {
            const int t = in.row_track[r];
            if (t >= 0 && (uint64_t)t < T) {
                const float *p = points + 4 * (uint64_t)t, *k = in.kps + 5 * r;
                const float pt[4] = {p[0], p[1], p[2], p[3]};
                is = rs_point_usable(pt, cmin) && tri_keypoint_usable(k[0], k[1]);
            }
            if (row_state) row_state[r] = is ? 1u : 0u;
        }
        block_compact(is, (unsigned)r, sc.idx, s_cnt, base);
    }
    if (tid == 0) sc.head[2 * (uint64_t)img] = (unsigned)(base - lo), sc.head[2 * (uint64_t)img + 1] = 1;
}

__global__ __launch_bounds__(kThreads) void rs_score(SceneTables in, const float *points, unsigned n_samples, unsigned seed,
                                                     double thr2, RsScratch sc) {
    __shared__ RsCorr s_c[kThreads];
    const unsigned img = blockIdx.x, tid = threadIdx.x, slice = blockIdx.z, slices = gridDim.z;
    const unsigned M = sc.head[2 * (uint64_t)img];
    if (M < 3 || (uint64_t)slice * kRsSliceLen >= M) return;                 // block-uniform (a non-candidate has M = 0)
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    float K[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];
    const unsigned c = blockIdx.y * kThreads + tid, k = c >> 2, j = c & 3;
    RsPose pose = {};
    bool valid = false;
    unsigned s[3];
    if (k < n_samples && sample3(seed + img, k, M, s)) {
        const RsCorr tri[3] = {load_corr(in, points, sc.idx[lo + s[0]]), load_corr(in, points, sc.idx[lo + s[1]]),
                               load_corr(in, points, sc.idx[lo + s[2]])};
        valid = rs_candidate_pose(tri, K, j, pose);
    }
    unsigned count = 0;
    for (uint64_t run = slice; run * kRsSliceLen < M; run += slices) {       // block-uniform
        const unsigned end = (unsigned)clamp_to((run + 1) * kRsSliceLen, M);
        for (unsigned p0 = (unsigned)(run * kRsSliceLen); p0 < end; p0 += kThreads) {
            __syncthreads();
            if (p0 + tid < end) s_c[tid] = load_corr(in, points, sc.idx[lo + p0 + tid]);
            __syncthreads();
            const unsigned n = end - p0 < (unsigned)kThreads ? end - p0 : (unsigned)kThreads;
            if (valid)
                for (unsigned q = 0; q < n; ++q) {
                    double e2;
                    count += rs_inlier(pose, K, s_c[q], thr2, e2) ? 1u : 0u;
                }
        }
    }
    if (valid) {
        count += slice == 0 ? 1u : 0u;
        if (count) atomicAdd(sc.votes + (uint64_t)img * 4 * n_samples + c, count);
    }
}

__global__ __launch_bounds__(kThreads) void rs_select(SceneTables in, const float *points, const float *poses, unsigned n_samples,
                                                      unsigned seed, double thr2, unsigned min_inliers, unsigned rounds, RsScratch sc,
                                                      float *poses_out,
                                                      unsigned *__restrict__ stats, float *__restrict__ err,
                                                      unsigned *__restrict__ row_state) {
    __shared__ double s_red[kWaves * (kRsTerms + 1)];
    __shared__ unsigned long long s_key[kWaves];
    __shared__ unsigned s_u[kWaves];
    const unsigned img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned M = sc.head[2 * (uint64_t)img];
    const bool cand = sc.head[2 * (uint64_t)img + 1] != 0;
    unsigned *st = stats + 4 * (uint64_t)img;
    float *po = poses_out + 12 * (uint64_t)img;
    if (!cand) {                                                             // block-uniform
        if (tid < 12) po[tid] = poses[12 * (uint64_t)img + tid];
        if (tid == 0) {
            st[0] = 0, st[1] = 0, st[2] = kRsNotCandidate, st[3] = kRsNone;
            if (err) err[2 * (uint64_t)img] = 0.f, err[2 * (uint64_t)img + 1] = 0.f;
        }
        return;
    }
    uint64_t lo, hi;
    image_range(in, img, lo, hi);
    float K[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = in.intrinsics[4 * (uint64_t)img + i];

    // the winner: the largest count, the lowest c on a tie, as the maximum of count << 32 | ~c
    unsigned long long key = 0;
    if (M >= 3)
        for (unsigned c = tid; c < 4 * n_samples; c += kThreads) {
            const unsigned v = sc.votes[(uint64_t)img * 4 * n_samples + c];
            const unsigned long long kk = (unsigned long long)v << 32 | (0xFFFFFFFFu - c);
            key = v && kk > key ? kk : key;
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        key = o > key ? o : key;
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) key = s_key[w] > key ? s_key[w] : key;
    const bool have = key != 0;
    const unsigned win = have ? 0xFFFFFFFFu - (unsigned)key : kRsNone;

    RsPose pose = {};
    if (have) {                                                              // block-uniform; every thread the same bits
        unsigned s[3];
        sample3(seed + img, win >> 2, M, s);
        const RsCorr tri[3] = {load_corr(in, points, sc.idx[lo + s[0]]), load_corr(in, points, sc.idx[lo + s[1]]),
                               load_corr(in, points, sc.idx[lo + s[2]])};
        rs_candidate_pose(tri, K, win & 3, pose);
    }

    // step 5: the refit rounds
    for (unsigned r = 0; have && r < rounds; ++r) {                          // block-uniform
        double acc[kRsTerms + 1];
#pragma unroll
        for (int i = 0; i <= kRsTerms; ++i) acc[i] = 0.0;
        for (unsigned p = tid; p < M; p += kThreads) {
            const RsCorr c = load_corr(in, points, sc.idx[lo + p]);
            double e2;
            const bool is = rs_inlier(pose, K, c, thr2, e2);
            acc[kRsTerms] = acc[kRsTerms] + (is ? e2 : thr2);
            if (is) {
                double w[kRsTerms];
                rs_gn_terms(pose, K, c, w);
#pragma unroll
                for (int i = 0; i < kRsTerms; ++i) acc[i] = acc[i] + w[i];
            }
        }
        block_sum<double, kRsTerms + 1>(acc, s_red);
        double d[6];
        if (!rs_cholesky6(acc, d)) break;
        RsPose next;
        rs_update(pose, d, next);
        double cost[1] = {0.0};
        for (unsigned p = tid; p < M; p += kThreads)
            cost[0] = cost[0] + rs_cost(next, K, load_corr(in, points, sc.idx[lo + p]), thr2);
        block_sum<double, 1>(cost, s_red);
        if (!(cost[0] <= acc[kRsTerms])) break;
        pose = next;
    }

    // step 7: the rounded pose's inliers
    TriObs o = {};
    rs_round(pose, K, o);
    double Xd[3];
    unsigned n_in[1] = {0};
    double e_sum[1] = {0.0}, e_max = 0.0;
    for (unsigned p = tid; have && p < M; p += kThreads) {
        const RsCorr c = load_corr(in, points, sc.idx[lo + p]);
        o.x = c.x, o.y = c.y;
        Xd[0] = double(c.X), Xd[1] = double(c.Y), Xd[2] = double(c.Z);
        double e2;
        if (tri_inlier(o, Xd, thr2, e2)) {
            n_in[0] += 1;
            e_sum[0] = e_sum[0] + e2;
            e_max = e2 > e_max ? e2 : e_max;
        }
    }
    block_sum<unsigned, 1>(n_in, s_u);
    block_sum<double, 1>(e_sum, s_red);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double other = __shfl_xor(e_max, m, 64);
        e_max = other > e_max ? other : e_max;
    }
    if (lane == 0) s_red[wave] = e_max;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) e_max = s_red[w] > e_max ? s_red[w] : e_max;
    const unsigned need = min_inliers > 3 ? min_inliers : 3;
    const bool posed = have && n_in[0] >= need;
    if (posed && row_state)
        for (unsigned p = tid; p < M; p += kThreads) {
            const unsigned row = sc.idx[lo + p];
            const RsCorr c = load_corr(in, points, row);
            o.x = c.x, o.y = c.y;
            Xd[0] = double(c.X), Xd[1] = double(c.Y), Xd[2] = double(c.Z);
            double e2;
            if (tri_inlier(o, Xd, thr2, e2)) row_state[row] = 2u;
        }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) po[i] = posed ? o.P[i] : 0.f;
        st[0] = M;
        st[1] = posed ? n_in[0] : 0u;
        st[2] = posed ? kRsPose : have ? kRsFewInliers : kRsNoCandidate;
        st[3] = win;
        if (err) {
            err[2 * (uint64_t)img] = posed ? float(sqrt(e_sum[0] / double(n_in[0]))) : 0.f;
            err[2 * (uint64_t)img + 1] = posed ? float(sqrt(e_max)) : 0.f;
        }
    }
}

uint64_t resect_scratch_bytes(unsigned n_images, uint64_t n_rows, unsigned n_samples) {
    return 4 * (n_rows + 2 * (uint64_t)n_images + 4 * (uint64_t)n_images * n_samples);
}

void launch_resect_cameras(void *scratch, const SceneTables &in, const float *points, const float *poses, double thr2, double cmin,
                           unsigned n_samples, unsigned min_inliers, unsigned rounds, unsigned seed, bool all, float *poses_out,
                           unsigned *stats, float *err, unsigned *row_state, hipStream_t stream) {
    const unsigned n_images = in.n_images;
    const uint64_t n_rows = in.n_rows;
    if (n_images == 0) return;
    unsigned *w = static_cast<unsigned *>(scratch);
    const RsScratch sc = {w, w + n_rows, w + n_rows + 2 * (uint64_t)n_images};
    const uint64_t runs = (n_rows + kRsSliceLen - 1) / kRsSliceLen;
    const unsigned slices = (unsigned)(runs < 1 ? 1 : runs > kRsMaxSlices ? kRsMaxSlices : runs);
    hipLaunchKernelGGL(rs_gather, dim3(n_images), dim3(kThreads), 0, stream, in, points, poses, n_samples, cmin, all ? 1u : 0u,
                       sc, row_state);
    hipLaunchKernelGGL(rs_score, dim3(n_images, (4 * n_samples + kThreads - 1) / kThreads, slices), dim3(kThreads), 0, stream, in,
                       points, n_samples, seed, thr2, sc);
    hipLaunchKernelGGL(rs_select, dim3(n_images), dim3(kThreads), 0, stream, in, points, poses, n_samples, seed, thr2, min_inliers,
                       rounds, sc, poses_out, stats, err, row_state);
}

}  // namespace lfmkd
