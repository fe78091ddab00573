// What the reconstruction stages share (mkd_triangulate.hip, mkd_resect.hip, mkd_bundle.hip, mkd_positions.hip): the tables of
// a scene as one struct from the entry layer to the kernels, and -- for the kernels -- the ONE device definition of the two
// canonical summation orders (include/lf_mkd.h; the host's are tri_combine in mkd_triangulate_math.h and
// rs_combine in mkd_resect_math.h) and of the walks the sums run over.  mkd_verify_common.h takes the workgroup sum from here,
// mkd_covisibility.hip and mkd_two_view_pose.hip the clamp.
#pragma once
#include <stdint.h>

namespace lfmkd {

// The tables of a scene, as the entry points of include/lf_mkd.h take them.  A stage that does not read a member gets it
// null or 0.  What is not a table -- points, poses, thresholds -- stays a kernel argument of its own.
struct SceneTables {
    const float *__restrict__ kps;             // [n_rows][5]: x, y read
    uint64_t n_rows;
    const uint64_t *__restrict__ off;          // [n_images + 1]: image offsets
    unsigned n_images;
    const uint64_t *__restrict__ toff;         // [tcap + 1]: track offsets
    uint64_t tcap;
    const int *__restrict__ obs_row;           // [ocap]
    const unsigned *__restrict__ obs_image;    // [ocap]
    uint64_t ocap;
    const unsigned *__restrict__ counts;       // {tracks, observations} the tables hold, each held to its capacity on the device
    const int *__restrict__ row_track;         // [n_rows]
    const float *__restrict__ intrinsics;      // [n_images][4]
};

#ifdef __HIPCC__
namespace {

// Every helper below is for workgroups of kSumThreads = 4 waves of 64: thread s is slot s of the 256-slot sum.  A file that sees
// kRsSlots (mkd_resect_math.h) asserts that the two are one number.  The sums are additions alone, and every file includes
// this header behind its *_math.h, under their contraction OFF.
constexpr int kSumThreads = 256, kSumWaves = kSumThreads / 64;

__device__ __forceinline__ uint64_t clamp_to(uint64_t v, uint64_t total) { return v < total ? v : total; }

// rows [lo, hi) of image img and positions [lo, hi) of track t (O: the observations the table holds), never decreasing and
// never beyond the total
__device__ __forceinline__ void image_range(const SceneTables &in, unsigned img, uint64_t &lo, uint64_t &hi) {
    lo = clamp_to(in.off[img], in.n_rows);
    hi = clamp_to(in.off[img + 1], in.n_rows);
    hi = hi > lo ? hi : lo;
}
__device__ __forceinline__ void track_range(const SceneTables &in, uint64_t t, uint64_t O, uint64_t &lo, uint64_t &hi) {
    lo = clamp_to(in.toff[t], O);
    hi = clamp_to(in.toff[t + 1], O);
    hi = hi > lo ? hi : lo;
}

// Workgroup sum of N values per thread in the 256-slot canonical order: the butterfly within a wave, then ((w0 + w1) + w2) + w3.
// Every thread gets the totals; `red` holds kSumWaves * N values.
template <typename T, int N>
__device__ __forceinline__ void block_sum(T *v, T *red) {
    static_assert(kSumWaves == 4, "the waves' partial sums are combined as ((w0 + w1) + w2) + w3");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T s = v[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, 64);
        if (lane == 0) red[wave * N + i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((red[i] + red[N + i]) + red[2 * N + i]) + red[3 * N + i];
    __syncthreads();
}
// the workgroup's total of an integer per thread (exact in any order)
__device__ __forceinline__ unsigned block_count(unsigned n, unsigned *s_cnt) {
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(s_cnt, n);
    __syncthreads();
    const unsigned total = *s_cnt;
    __syncthreads();
    return total;
}
// one integer add per wave for a per-lane predicate
__device__ __forceinline__ void count_wave(bool p, unsigned *word) {
    const unsigned long long bits = __ballot(p);
    if ((threadIdx.x & 63) == 0 && bits) atomicAdd(word, (unsigned)__popcll(bits));
}
// One step of the ordered workgroup compaction: the threads hold 256 consecutive entries of an ascending walk, `is` says which
// are kept, and the kept entries' values go to dst[base], dst[base + 1], .. in the walk's order (ballot, popcount, the waves'
// counts through s_cnt [kSumWaves]: no atomic decides a position); base moves past them.  Block-uniform control flow only:
// two barriers, one before the counts are read and one behind the store, before s_cnt is written again.
__device__ __forceinline__ void block_compact(bool is, unsigned value, unsigned *dst, unsigned *s_cnt, uint64_t &base) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t bits = __ballot(is);
    if (lane == 0) s_cnt[wave] = (unsigned)__popcll(bits);
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSumWaves; ++w) {
        before += (unsigned)w < wave ? s_cnt[w] : 0u;
        total += s_cnt[w];
    }
    if (is) dst[base + before + (unsigned)__popcll(bits & ((1ull << lane) - 1ull))] = value;
    base += total;
    __syncthreads();
}

// ---- the per-track walk: behind mkd_triangulate_math.h alone, whose kTriSlots is the number of lanes that own a track ------------
#ifdef LF_TRI_SLOTS
// the butterfly of the 4-slot canonical sum over the group's lanes: (s0 + s2) + (s1 + s3) in every lane
__device__ __forceinline__ double combine(double v) {
#pragma unroll
    for (int m = kTriSlots / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}
// the group's bits of a ballot (base: the group's first lane)
__device__ __forceinline__ unsigned group_bits(bool p, unsigned base) {
    return (unsigned)(__ballot(p) >> base) & ((1u << kTriSlots) - 1u);
}
// What a per-track kernel knows of where it is: T, O, its wave's first track and stride, its lane's slot and its group's first
// lane.  The walk is `for (t0 = first; t0 < T; t0 += stride)` with t = t0 + lane / kTriSlots: wave-uniform.
struct TrackWalk {
    uint64_t T, O, first, stride;
    unsigned l, base;
};
__device__ __forceinline__ TrackWalk track_walk(const SceneTables &in) {
    TrackWalk w;
    w.T = clamp_to(in.counts[0], in.tcap);
    w.O = clamp_to(in.counts[1], in.ocap);
    const unsigned lane = threadIdx.x & 63;
    w.l = lane & (kTriSlots - 1);
    w.base = lane & ~(unsigned)(kTriSlots - 1);
    w.first = ((uint64_t)blockIdx.x * kSumWaves + (threadIdx.x >> 6)) * (64 / kTriSlots);
    w.stride = (uint64_t)gridDim.x * kSumWaves * (64 / kTriSlots);
    return w;
}
#endif

}  // namespace
#endif

}  // namespace lfmkd
