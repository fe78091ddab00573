// gfx950 covisibility tables (include/lf_mkd.h, lf_mkd_covisibility_device): per pair of images the number of
// tracks of a track table (lf_mkd_track_table_device's d_track_offsets / d_obs_image / d_counts) that both see.
//
//   cv_zero    zeroes the table (not under LF_MKD_COVIS_ACCUMULATE) and the scratch's chunk bitmap (always);
//   cv_short   a GROUP of G lanes (4 .. 64, the plan's form) per track: the track's positions G at a time, one per lane; for
//              every pair of chunks (A, B >= A) the COUNTED lanes of A are visited one by one (the set bits of a ballot), their
//              image is broadcast in the group (ds_bpermute) and every counted lane of B adds one pair -- so a step of the loop
//              makes up to G adds (2 G between different chunks: both orders), and a consistent track of L images costs
//              L ceil(L / G) steps of full lanes.  Tracks of more than kLongChunks G positions are not counted here: the group
//              marks their 64-position chunks of the observation array in the bitmap instead;
//   cv_long    a wave per marked 64-position chunk of the observation array: every lane finds the track of its position (a
//              binary search in the offsets), and for each long track in the chunk (at most two for offsets that do not
//              decrease) the wave walks the whole track 64 positions at a time against its own counted lanes.  Only lanes
//              that are counted cost a step, so ONE track of every row made without LF_MKD_TRACK_TABLE_CONSISTENT -- L positions,
//              D distinct images -- costs at most D ceil(L / 64) steps and ceil(L / 64) loads in each of at most D waves: the
//              bound is (distinct images) x (track length), never length squared;
//   cv_mask    one thread per edge: both entries of the pair to 0.
//
// Integer atomic adds only (global_atomic_add_u32 without return), so the table is exact and independent of the run, the CU
// count and the form.  With few images every add lands on a handful of words: up to kLdsImages images a workgroup of cv_short
// counts into a private n x n table in LDS and adds its non-zero entries to the global table once, at its end (consecutive
// lanes, consecutive words: those adds reach L2 a cache line at a time, the scattered ones of the direct form one by one).
// NOBODY WAITS: no flag, no spin; the bitmap is written by cv_short and read by cv_long, a launch later.
// Every loop that holds a ballot or a lane permute runs in wave-uniform control flow: a group that has nothing left goes
// through the steps with its predicate off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_scene.h"   // clamp_to

#ifndef LF_COVIS_LDS_IMAGES
#define LF_COVIS_LDS_IMAGES 64      // the largest n_images that counts in LDS first; 0 builds the plan without that form
#endif

namespace lfmkd {
namespace {

constexpr int kThreads = 256;
constexpr unsigned kLongChunks = 16;                    // a track of more than kLongChunks G positions is cv_long's
constexpr unsigned kLdsImages = LF_COVIS_LDS_IMAGES;
constexpr unsigned kMaxBlocks = 4096;                   // grid-stride beyond: 16 workgroups a CU
static_assert(kLdsImages <= 64, "the private table is at most 16 KiB");

template <bool LDS>
__device__ __forceinline__ void add_pair(unsigned *covis, unsigned *tab, unsigned n, unsigned i, unsigned j) {
    if (LDS) atomicAdd(tab + i * n + j, 1u);
    else atomicAdd(covis + (size_t)i * n + j, 1u);
}

// is position k of a track that starts at lo counted?  (the raw neighbour first, then the range test)
__device__ __forceinline__ bool counted(const unsigned *__restrict__ img, uint64_t k, uint64_t lo, unsigned v, unsigned n) {
    return (k == lo || v != img[k - 1]) && v < n;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void cv_zero(unsigned *__restrict__ covis, uint64_t entries, unsigned *__restrict__ bitmap,
                                                    uint64_t bitmap_words) {
    const uint64_t step = (uint64_t)gridDim.x * kThreads;
    const uint64_t first = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (uint64_t i = first; i < entries; i += step) covis[i] = 0u;
    for (uint64_t i = first; i < bitmap_words; i += step) bitmap[i] = 0u;
}

template <int G, bool LDS>
__global__ __launch_bounds__(kThreads) void cv_short(const uint64_t *__restrict__ off, uint64_t track_capacity,
                                                     const unsigned *__restrict__ img, uint64_t obs_capacity,
                                                     const unsigned *__restrict__ counts, unsigned n, unsigned *__restrict__ covis,
                                                     unsigned *__restrict__ bitmap) {
    __shared__ unsigned tab[LDS && kLdsImages ? kLdsImages * kLdsImages : 1];
    if (LDS) {
        for (unsigned i = threadIdx.x; i < n * n; i += kThreads) tab[i] = 0u;
        __syncthreads();
    }
    const uint64_t T = clamp_to(counts[0], track_capacity), O = clamp_to(counts[1], obs_capacity);
    constexpr unsigned kPerWave = 64 / G;
    constexpr uint64_t kGroupMask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1;
    const unsigned lane = threadIdx.x & 63, l = lane & (G - 1), base = lane & ~(unsigned)(G - 1);
    const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint64_t waves = (uint64_t)gridDim.x * (kThreads / 64);
    for (uint64_t t0 = wave * kPerWave; t0 < T; t0 += waves * kPerWave) {       // wave-uniform
        const uint64_t t = t0 + lane / G;
        uint64_t lo = 0, hi = 0;
        if (t < T) {
            lo = clamp_to(off[t], O);
            hi = clamp_to(off[t + 1], O);
        }
        uint64_t len = hi > lo ? hi - lo : 0;
        if (len > (uint64_t)kLongChunks * G) {                                   // cv_long's: mark its chunks of the array
            for (uint64_t c = (lo >> 6) + l; c <= ((hi - 1) >> 6); c += G) atomicOr(bitmap + (c >> 5), 1u << (c & 31));
            len = 0;
        }
        const unsigned nch = (unsigned)((len + G - 1) / G);
        for (unsigned ca = 0; __any(ca < nch); ++ca) {
            const uint64_t pa = lo + (uint64_t)ca * G + l;
            const bool in_a = ca < nch && pa < hi;
            const unsigned ia = in_a ? img[pa] : 0xFFFFFFFFu;
            const bool c_a = in_a && counted(img, pa, lo, ia, n);
            const uint64_t mask_a = (__ballot(c_a) >> base) & kGroupMask;
            for (unsigned cb = ca; __any(cb < nch && mask_a != 0); ++cb) {
                const uint64_t pb = lo + (uint64_t)cb * G + l;
                const bool in_b = cb < nch && pb < hi;
                const unsigned ib = in_b ? img[pb] : 0xFFFFFFFFu;
                const bool c_b = in_b && counted(img, pb, lo, ib, n);
                uint64_t m = mask_a;
                while (__any(m != 0)) {
                    const bool live = m != 0;
                    const unsigned s = live ? (unsigned)__ffsll((unsigned long long)m) - 1u : 0u;
                    m &= m - 1;
                    const unsigned src = (unsigned)__shfl((int)ia, (int)(base + s), 64);
                    if (live && c_b) {
                        if (cb == ca) {
                            if (src != ib || s == l) add_pair<LDS>(covis, tab, n, src, ib);
                        } else if (src != ib) {
                            add_pair<LDS>(covis, tab, n, src, ib);
                            add_pair<LDS>(covis, tab, n, ib, src);
                        }
                    }
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (unsigned i = threadIdx.x; i < n * n; i += kThreads)
            if (const unsigned v = tab[i]) atomicAdd(covis + i, v);
    }
}

// One wave per 64 positions of the observation array whose bit cv_short set.  `long_min`: kLongChunks G of cv_short's form.
__global__ __launch_bounds__(kThreads) void cv_long(const uint64_t *__restrict__ off, uint64_t track_capacity,
                                                    const unsigned *__restrict__ img, uint64_t obs_capacity,
                                                    const unsigned *__restrict__ counts, unsigned n, unsigned *__restrict__ covis,
                                                    const unsigned *__restrict__ bitmap, uint64_t long_min) {
    const uint64_t T = clamp_to(counts[0], track_capacity), O = clamp_to(counts[1], obs_capacity);
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint64_t waves = (uint64_t)gridDim.x * (kThreads / 64);
    const uint64_t chunks = (O + 63) >> 6;
    for (uint64_t c = wave; c < chunks; c += waves) {                            // wave-uniform
        if (!((bitmap[c >> 5] >> (c & 31)) & 1u)) continue;
        const uint64_t k = (c << 6) + lane;
        // the last track whose (clamped) start is at or before k
        uint64_t a = 0, b = T;
        while (a < b) {
            const uint64_t mid = a + ((b - a) >> 1);
            if (clamp_to(off[mid], O) <= k) a = mid + 1;
            else b = mid;
        }
        uint64_t t = 0, lo = 0, hi = 0;
        bool mine = false;
        if (k < O && a > 0) {
            t = a - 1;
            lo = clamp_to(off[t], O);
            hi = clamp_to(off[t + 1], O);
            mine = lo <= k && k < hi && hi - lo > long_min;
        }
        const unsigned ia = mine ? img[k] : 0xFFFFFFFFu;
        const bool c_a = mine && counted(img, k, lo, ia, n);
        uint64_t pending = __ballot(c_a);
        while (pending) {                                                         // one round per long track in the chunk
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const uint64_t tl = __shfl((unsigned long long)t, leader, 64);
            const uint64_t lo_l = __shfl((unsigned long long)lo, leader, 64), hi_l = __shfl((unsigned long long)hi, leader, 64);
            const uint64_t mask = __ballot(c_a && t == tl);
            pending &= ~mask;
            for (uint64_t q0 = lo_l; q0 < hi_l; q0 += 64) {
                const uint64_t q = q0 + lane;
                const bool in_b = q < hi_l;
                const unsigned ib = in_b ? img[q] : 0xFFFFFFFFu;
                const bool c_b = in_b && counted(img, q, lo_l, ib, n);
                if (!__ballot(c_b)) continue;
                for (uint64_t m = mask; m; m &= m - 1) {
                    const int s = __ffsll((unsigned long long)m) - 1;
                    const unsigned src = (unsigned)__shfl((int)ia, s, 64);
                    if (c_b && (src != ib || (c << 6) + (unsigned)s == q)) atomicAdd(covis + (size_t)src * n + ib, 1u);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void cv_mask(const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                    uint64_t n_edges, unsigned n, unsigned *__restrict__ covis) {
    const uint64_t step = (uint64_t)gridDim.x * kThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < n_edges; e += step) {
        const unsigned a = edge_a[e], b = edge_b[e];
        if (a < n && b < n) {
            covis[(size_t)a * n + b] = 0u;
            covis[(size_t)b * n + a] = 0u;
        }
    }
}

CovisibilityPlan covisibility_plan(unsigned n_images, uint64_t track_capacity, uint64_t obs_capacity, uint64_t n_edges) {
    CovisibilityPlan p = {};
    if (n_images == 0) return p;
    const bool count = track_capacity && obs_capacity;
    // lanes per track: enough for twice the mean length the capacities allow, never more than the images there are
    const uint64_t mean = count ? (obs_capacity + track_capacity - 1) / track_capacity : 1;
    const uint64_t want = 2 * mean < n_images ? 2 * mean : n_images;
    p.group = 4;
    while (p.group < 64 && p.group < want) p.group *= 2;
    p.lds = kLdsImages && n_images <= kLdsImages;
    const auto blocks = [](uint64_t threads) {
        const uint64_t b = (threads + kThreads - 1) / kThreads;
        return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
    };
    p.zero_blocks = blocks(((uint64_t)n_images * n_images + 3) / 4);
    p.bitmap_words = count ? (obs_capacity + 2047) / 2048 : 0;
    p.short_blocks = count ? blocks(track_capacity * p.group) : 0;
    if (p.lds) {                                        // every workgroup adds its n^2 words at its end: at most 2^22 of them
        const unsigned cap = (1u << 22) / (n_images * n_images);
        if (p.short_blocks > (cap > 256 ? cap : 256)) p.short_blocks = cap > 256 ? cap : 256;
    }
    p.long_blocks = count ? blocks(obs_capacity) : 0;
    p.mask_blocks = n_edges ? blocks(n_edges) : 0;
    p.launches = 1 + (count ? 2 : 0) + (n_edges ? 1 : 0);
    p.scratch_bytes = p.bitmap_words * 4;
    return p;
}

template <int G>
static void launch_short(const CovisibilityPlan &p, const uint64_t *off, uint64_t track_capacity, const unsigned *img,
                         uint64_t obs_capacity, const unsigned *counts, unsigned n, unsigned *covis, unsigned *bitmap,
                         hipStream_t stream) {
    if (p.lds)
        hipLaunchKernelGGL((cv_short<G, true>), dim3(p.short_blocks), dim3(kThreads), 0, stream, off, track_capacity, img,
                           obs_capacity, counts, n, covis, bitmap);
    else
        hipLaunchKernelGGL((cv_short<G, false>), dim3(p.short_blocks), dim3(kThreads), 0, stream, off, track_capacity, img,
                           obs_capacity, counts, n, covis, bitmap);
}

void launch_covisibility(const CovisibilityPlan &p, unsigned char *scratch, const uint64_t *off, uint64_t track_capacity,
                         const unsigned *img, uint64_t obs_capacity, const unsigned *counts, unsigned n, const unsigned *edge_a,
                         const unsigned *edge_b, uint64_t n_edges, bool accumulate, unsigned *covis, hipStream_t stream) {
    if (n == 0) return;
    unsigned *bitmap = reinterpret_cast<unsigned *>(scratch);
    hipLaunchKernelGGL(cv_zero, dim3(p.zero_blocks), dim3(kThreads), 0, stream, covis, accumulate ? 0 : (uint64_t)n * n, bitmap,
                       p.bitmap_words);
    if (p.short_blocks) {
        switch (p.group) {
            case 4: launch_short<4>(p, off, track_capacity, img, obs_capacity, counts, n, covis, bitmap, stream); break;
            case 8: launch_short<8>(p, off, track_capacity, img, obs_capacity, counts, n, covis, bitmap, stream); break;
            case 16: launch_short<16>(p, off, track_capacity, img, obs_capacity, counts, n, covis, bitmap, stream); break;
            case 32: launch_short<32>(p, off, track_capacity, img, obs_capacity, counts, n, covis, bitmap, stream); break;
            default: launch_short<64>(p, off, track_capacity, img, obs_capacity, counts, n, covis, bitmap, stream); break;
        }
        hipLaunchKernelGGL(cv_long, dim3(p.long_blocks), dim3(kThreads), 0, stream, off, track_capacity, img, obs_capacity,
                           counts, n, covis, bitmap, (uint64_t)kLongChunks * p.group);
    }
    if (n_edges) hipLaunchKernelGGL(cv_mask, dim3(p.mask_blocks), dim3(kThreads), 0, stream, edge_a, edge_b, n_edges, n, covis);
}

}  // namespace lfmkd
