// gfx950 edge-list matching over 8-bit descriptors (include/lf_mkd.h, "edge lists"): any pairs of images from
// one pool in one launch, no row copied.
//
// A POOL is a row array plus image_offsets [n_images + 1]: image m owns rows [image_offsets[m], image_offsets[m + 1]), read
// through pair_rows against the pool's total.  An EDGE e is (edge_a[e], edge_b[e]), two image ids; an id at or beyond
// n_images names an empty image.  The EDGE LAYOUT of one side is an ordinary pair layout -- edge_offsets [n_edges + 1] with
// edge_offsets[e + 1] - edge_offsets[e] = the rows of that side's image of edge e -- and everything indexed "like a" lives in
// it, so the mutual filter, the verifiers and the guided calls take it as it is.
//
//   edge_layout       the exclusive prefix sum of the edges' row counts (two launches, one when a single block does it);
//   gather_edge_rows  rows of any width from the pool into the edge layout (how keypoints reach the verifiers);
//   match_q8_edges    match_q8_pairs' body (mkd_match_q8_batched.h) behind a prologue that takes the slot and the output base
//                     from the edge layout and x / y from the pools through the edge's two ids.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_match_small.h"       // pair_rows, image_rows, last_pair_at_or_before
#include "mkd_match_q8_batched.h"  // q8_edges_slot, q8_pairs_block, the batched form's kP* shape

namespace lfmkd {
namespace {

constexpr int kLayoutThreads = 256, kLayoutPer = 4;
constexpr int kLayoutBlock = kLayoutThreads * kLayoutPer;   // edges one workgroup of edge_layout scans
constexpr uint64_t kPartial = 1ull << 63;                   // a block's own sum, not yet the prefix (sums stay below 2^63)
constexpr int kGatherRows = 64, kGatherThreads = 256;       // rows one workgroup of gather_edge_rows copies

}  // namespace

// Both launches of the layout.  Workgroup k scans edges [k B, (k + 1) B), B = kLayoutBlock.
//   pass 0 (only when there is more than one workgroup): the block's own sum T_k, tagged with kPartial, goes to the block's
//          last entry, out[min((k + 1) B, n_edges)]; nothing else is written.
//   pass 1: the block's base is the sum of the T_j in front of it, then every entry of the block is written.  The base is read
//          from those same last entries, which the blocks in front overwrite with their final values during this very launch:
//          an entry still tagged is T_j, an entry no longer tagged is the whole prefix up to and including block j.  Either
//          reading is usable and each entry is read once, so the base is  (the nearest untagged entry, or 0) + the tagged
//          entries behind it  whatever the order the blocks run in -- nobody waits for anybody.
__global__ __launch_bounds__(kLayoutThreads) void edge_layout(const uint64_t *__restrict__ image_off, unsigned n_images,
                                                              uint64_t total, const unsigned *__restrict__ edge_image,
                                                              unsigned n_edges, uint64_t *out, int pass) {
    __shared__ uint64_t s_sum[kLayoutThreads];
    __shared__ long long s_near[kLayoutThreads];
    const unsigned k = blockIdx.x, t = threadIdx.x;
    const uint64_t e0 = (uint64_t)k * kLayoutBlock + (uint64_t)t * kLayoutPer;
    uint64_t rows[kLayoutPer], mine = 0;
#pragma unroll
    for (int i = 0; i < kLayoutPer; ++i) {
        long lo, n = 0;
        if (e0 + i < n_edges) image_rows(image_off, n_images, total, edge_image[e0 + i], lo, n);
        rows[i] = (uint64_t)n;
        mine += rows[i];
    }
    // inclusive scan of the threads' sums
    s_sum[t] = mine;
    __syncthreads();
    for (int d = 1; d < kLayoutThreads; d <<= 1) {
        const uint64_t v = t >= (unsigned)d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    const uint64_t before = s_sum[t] - mine, block_sum = s_sum[kLayoutThreads - 1];
    const uint64_t last = (uint64_t)(k + 1) * kLayoutBlock < n_edges ? (uint64_t)(k + 1) * kLayoutBlock : n_edges;
    if (pass == 0) {
        if (t == 0) __hip_atomic_store(out + last, block_sum | kPartial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // the base: one reading of every earlier block's last entry, kLayoutThreads of them at a time from the nearest back
    uint64_t base = 0;
    for (long long top = (long long)k - 1; top >= 0; top -= kLayoutThreads) {   // (the same for the whole workgroup)
        const long long j = top - t;
        uint64_t v = kPartial;                                  // in front of block 0: a tagged zero
        if (j >= 0) v = __hip_atomic_load(out + (uint64_t)(j + 1) * kLayoutBlock, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        s_near[t] = (v & kPartial) ? -1 : j;
        __syncthreads();
        for (int d = kLayoutThreads / 2; d > 0; d >>= 1) {
            if (t < (unsigned)d) s_near[t] = s_near[t] > s_near[t + d] ? s_near[t] : s_near[t + d];
            __syncthreads();
        }
        const long long nearest = s_near[0];                    // the nearest untagged entry of these, -1: none
        // the entries behind it are all tagged: their sums, and the prefix it holds itself
        s_sum[t] = (j < 0 || j < nearest) ? 0 : (j == nearest ? v : (v & ~kPartial));
        __syncthreads();
        for (int d = kLayoutThreads / 2; d > 0; d >>= 1) {
            if (t < (unsigned)d) s_sum[t] += s_sum[t + d];
            __syncthreads();
        }
        base += s_sum[0];
        if (nearest >= 0) break;
    }
    if (k == 0 && t == 0) out[0] = 0;
    uint64_t run = base + before;
#pragma unroll
    for (int i = 0; i < kLayoutPer; ++i) {
        run += rows[i];
        if (e0 + i < n_edges) {
            if (e0 + i + 1 == last) __hip_atomic_store(out + last, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else out[e0 + i + 1] = run;
        }
    }
}

// dst row lo + r = src row first + r for r < min(n, len): (lo, len) the edge's range of the layout against the capacity,
// (first, n) its image's rows.  Both runs are contiguous, so a workgroup copies kGatherRows rows as one run of dwords.  The
// grid is the matcher's slot map at kGatherRows rows a slot: floor(capacity / kGatherRows) + n_edges workgroups.
__global__ __launch_bounds__(kGatherThreads) void gather_edge_rows(const unsigned *__restrict__ src, unsigned row_words,
                                                                   const uint64_t *__restrict__ image_off, unsigned n_images,
                                                                   uint64_t total, const unsigned *__restrict__ edge_image,
                                                                   const uint64_t *__restrict__ edge_off, uint64_t capacity,
                                                                   unsigned n_edges, unsigned *__restrict__ dst) {
    const uint64_t slot = blockIdx.x;
    auto start = [&](unsigned p) { return (edge_off[p] < capacity ? edge_off[p] : capacity) / kGatherRows + p; };
    const unsigned p = last_pair_at_or_before(n_edges, slot, start);
    long lo, len, first, n;
    pair_rows(edge_off[p], edge_off[p + 1], capacity, lo, len);
    const long block = (long)slot - (lo / kGatherRows + (long)p);
    if (block < 0) return;                                       // rows in front of the first edge
    image_rows(image_off, n_images, total, edge_image[p], first, n);
    n = n < len ? n : len;
    const long r0 = block * kGatherRows;
    if (r0 >= n) return;                                         // the edge's idle slot(s)
    const long r1 = r0 + kGatherRows < n ? r0 + kGatherRows : n;
    const unsigned *s = src + (first + r0) * row_words;
    unsigned *d = dst + (lo + r0) * row_words;
    const long words = (r1 - r0) * row_words;
    for (long w = threadIdx.x; w < words; w += kGatherThreads) d[w] = s[w];
}

// ---- match_q8_edges (lf_mkd_match_q8_edges_device) -----------------------------------------------------------------------
// match_q8_pairs' body (q8_pairs_block, mkd_match_q8_batched.h) behind the edges prologue (q8_edges_slot, the same header,
// with the notes on what it serves and on the clamps): the two IMAGES of the edge are the body's whole problem.
__global__ __launch_bounds__(kPThreads) void match_q8_edges(
    const unsigned char *__restrict__ a, const uint64_t *__restrict__ image_off_a, unsigned n_images_a, uint64_t na_total,
    const unsigned char *__restrict__ b, const uint64_t *__restrict__ image_off_b, unsigned n_images_b, uint64_t nb_total,
    const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b, const uint64_t *__restrict__ edge_off_a,
    uint64_t ea_capacity, const uint64_t *__restrict__ edge_off_b, uint64_t eb_capacity, unsigned n_edges, unsigned slots_ab,
    float ratio, int *__restrict__ match_ab, int *__restrict__ match_ba, int *__restrict__ best_out,
    int *__restrict__ second_out) {
    __shared__ __attribute__((aligned(16))) unsigned char s_y[2][kPStage * kQTileBytes];
    Q8Slot s;
    if (!q8_edges_slot(image_off_a, n_images_a, na_total, image_off_b, n_images_b, nb_total, edge_a, edge_b, edge_off_a, ea_capacity,
                       edge_off_b, eb_capacity, n_edges, slots_ab, s))
        return;                                                  // an idle slot
    int *match = (s.rev ? match_ba : match_ab) + s.out_lo;
    int *best_o = s.rev || !best_out ? nullptr : best_out + s.out_lo;
    int *second_o = s.rev || !second_out ? nullptr : second_out + s.out_lo;
    if (s.ny < 2) {                                              // a side the single-pair call refuses
        q8_fill_none(match, best_o, second_o, s.block, s.nx);
        return;
    }
    const unsigned char *x = (s.rev ? b : a) + s.x_lo * 128, *y = (s.rev ? a : b) + s.y_lo * 128;
    q8_pairs_block(x, s.nx, y, s.ny, ratio, match, best_o, second_o, s.block, s_y);
}

unsigned gather_edge_rows_block_rows() { return kGatherRows; }

void launch_edge_layout(const uint64_t *image_off, unsigned n_images, uint64_t total, const unsigned *edge_image,
                        unsigned n_edges, uint64_t *edge_off, hipStream_t stream) {
    if (n_edges == 0) return;
    const unsigned blocks = (unsigned)(((uint64_t)n_edges + kLayoutBlock - 1) / kLayoutBlock);
    for (int pass = blocks > 1 ? 0 : 1; pass < 2; ++pass)
        hipLaunchKernelGGL(edge_layout, dim3(blocks), dim3(kLayoutThreads), 0, stream, image_off, n_images, total, edge_image,
                           n_edges, edge_off, pass);
}

void launch_gather_edge_rows(const void *src, unsigned row_bytes, const uint64_t *image_off, unsigned n_images, uint64_t total,
                             const unsigned *edge_image, const uint64_t *edge_off, uint64_t capacity, unsigned n_edges, void *dst,
                             hipStream_t stream) {
    if (n_edges == 0) return;
    const uint64_t slots = capacity / kGatherRows + n_edges;
    hipLaunchKernelGGL(gather_edge_rows, dim3((unsigned)slots), dim3(kGatherThreads), 0, stream,
                       static_cast<const unsigned *>(src), row_bytes / 4, image_off, n_images, total, edge_image, edge_off,
                       capacity, n_edges, static_cast<unsigned *>(dst));
}

void launch_match_q8_edges(const unsigned char *a, const uint64_t *image_off_a, unsigned n_images_a, uint64_t na_total,
                           const unsigned char *b, const uint64_t *image_off_b, unsigned n_images_b, uint64_t nb_total,
                           const unsigned *edge_a, const unsigned *edge_b, const uint64_t *edge_off_a, uint64_t ea_capacity,
                           const uint64_t *edge_off_b, uint64_t eb_capacity, unsigned n_edges, float ratio, bool mutual,
                           int *match_ab, int *match_ba, int *best, int *second, hipStream_t stream) {
    if (n_edges == 0) return;
    const uint64_t slots_ab = match_q8_pairs_slots(ea_capacity, n_edges);
    const uint64_t slots = slots_ab + (match_ba ? match_q8_pairs_slots(eb_capacity, n_edges) : 0);
    hipLaunchKernelGGL(match_q8_edges, dim3((unsigned)slots), dim3(kPThreads), 0, stream, a, image_off_a, n_images_a, na_total,
                       b, image_off_b, n_images_b, nb_total, edge_a, edge_b, edge_off_a, ea_capacity, edge_off_b, eb_capacity,
                       n_edges, (unsigned)slots_ab, ratio, match_ab, match_ba, best, second);
    if (mutual) launch_match_mutual(edge_off_a, ea_capacity, edge_off_b, eb_capacity, n_edges, match_ab, match_ba, stream);
}

}  // namespace lfmkd
