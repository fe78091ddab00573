// gfx950 k-nearest-neighbour search over 8-bit descriptors: the exact top-k (include/lf_mkd.h, lf_mkd_knn_q8_device;
// DESIGN.md 6h).
//
// `match_q8_scan` of mkd_match_q8.hip with another epilogue.  Everything in front of it is that kernel's: the a fragments in
// registers (XORed once), b straight from the caller's rows by per-lane LDS-DMA into the [chunk 8][row 32][16 B] tile image
// (XOR after the read), kNStage tiles per barrier, double buffered, vmcnt(0) plus a barrier per stage, four
// v_mfma_i32_32x32x32_i8 per 32 x 32 tile of pairs, the clamps on the DMA address (nb - 1) and on idle a rows (na - 1), masked
// candidates at INT32_MIN.  No request leaves [0, na) / [0, nb).
//
// The epilogue keeps, per lane and a tile, the K best candidates of the lane's column, sorted, in 2 K registers.  The order is
// that of ONE 64-bit key per candidate,
//     key = (s + 2^21) << 32 | row            (|s| <= 128 * 127^2 = 2 064 512 < 2^21, so the high word is 1 .. 2^22 - 1)
// "larger key first" IS the contract's order (larger s first, among equal s the higher index first); a row occurs once per a
// row, so keys are unique; key 0 is "none" and sorts behind every candidate.  The fold of the two lane halves and the merge of
// the splits are max-merges of such keys, so their result cannot depend on the order in which the lists arrive: not on the
// split count, not on the CU count.  During the scan the list is held as (score, row) pairs instead: lane (r, h) owns a
// column and, per b tile, the 16 rows 32 t + 4 h + (i & 3) + 8 (i >> 2), ascending in i and in t, so a new candidate has a
// higher index than anything the lane holds and the key comparison reduces to the 32-bit  v >= score[j]  -- one compare and
// four selects per slot (knn_insert_ascending).  The lists are only ever indexed statically (unrolled), so they stay in
// registers: no instantiation uses scratch memory.
//
// The insertion is gated as the top-2 code gates its own: the tile's 16 values are reduced with v_max3_i32 and the wave asks
// ballot(m >= kth && m != INT_MIN), kth = the score of the list's K-th entry (INT_MIN while the list is not full).  `>=`, not
// `>`: an equal score arrives at a higher index and displaces.  Inside, each of the 16 values is gated once more before its
// K-step insertion.
//
// Grid = (a blocks of kNBlockRows rows, b splits).  With one split the scan writes index / score itself; otherwise it writes
// each row's k keys for its split, and `knn_q8_merge` max-merges the splits' lists (in ascending split order, which by the
// above does not matter).  k is served by the next compiled K (2, 4, 8, 16); only k columns are ever written.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_match_q8_common.h"   // the tile constants, q8_lds_dma16, max3i

// the workgroup (measured beside 8 x 2 and 4 x 1)
#ifndef LF_Q8_KNN_WAVES
#define LF_Q8_KNN_WAVES 8
#endif
#ifndef LF_Q8_KNN_TILES
#define LF_Q8_KNN_TILES 1
#endif

namespace lfmkd {
namespace {

constexpr int kNWaves = LF_Q8_KNN_WAVES, kNTiles = LF_Q8_KNN_TILES;
constexpr int kNThreads = 64 * kNWaves;
constexpr int kNStage = 4;                                   // b tiles per LDS stage: 16 KiB
constexpr int kNPieces = kNStage * 256 / kNThreads;          // 16-byte DMA pieces per thread and stage
constexpr int kNBlockRows = kNWaves * kNTiles * kQTileRows;
constexpr int kNMaxSplits = 1024;
constexpr int kKeyBias = 1 << 21;
static_assert(kNPieces * kNThreads == kNStage * 256 && kNPieces >= 1, "whole pieces");

__device__ __forceinline__ unsigned long long knn_key(int s, unsigned row) {
    return (unsigned long long)(unsigned)(s + kKeyBias) << 32 | row;
}
__device__ __forceinline__ int knn_key_score(unsigned long long key) { return key ? (int)(key >> 32) - kKeyBias : INT_MIN; }
__device__ __forceinline__ int knn_key_index(unsigned long long key) { return key ? (int)(unsigned)key : -1; }

// key into the descending list: list[j] = max(list[j], min(list[j - 1], key)), from the tail up
template <int K>
__device__ __forceinline__ void knn_insert(unsigned long long (&list)[K], unsigned long long key) {
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        const unsigned long long up = list[j - 1] < key ? list[j - 1] : key;
        list[j] = list[j] > up ? list[j] : up;
    }
    list[0] = list[0] > key ? list[0] : key;
}

// The scan's own insertion, on the list kept as (score, row) pairs: a lane meets its rows in ascending order, so a new
// candidate has a higher index than anything the lane holds and "enters above slot j" is the 32-bit test v >= score[j]
// (an empty slot holds INT_MIN / -1; `valid` keeps a masked value out).  One compare and four selects per slot; the result is
// the list knn_insert would give on the keys.
template <int K>
__device__ __forceinline__ void knn_insert_ascending(int (&score)[K], int (&row)[K], int v, int r, bool valid) {
    bool above[K];
#pragma unroll
    for (int j = 0; j < K; ++j) above[j] = valid && v >= score[j];
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        score[j] = above[j - 1] ? score[j - 1] : (above[j] ? v : score[j]);
        row[j] = above[j - 1] ? row[j - 1] : (above[j] ? r : row[j]);
    }
    score[0] = above[0] ? v : score[0];
    row[0] = above[0] ? r : row[0];
}

}  // namespace

// final != 0 (one split): index_out / score_out [na][k] are written here and part is not used.
// part: [split][c < k][na] keys
template <int K>
__global__ __launch_bounds__(kNThreads) void knn_q8_scan(const unsigned char *__restrict__ a, long na,
                                                          const unsigned char *__restrict__ b, long nb, long tiles_per_split,
                                                          const unsigned *__restrict__ excl_lo,
                                                          const unsigned *__restrict__ excl_hi,
                                                          unsigned long long *__restrict__ part, int final, int k,
                                                          int *__restrict__ index_out, int *__restrict__ score_out) {
    __shared__ __attribute__((aligned(16))) unsigned char s_b[2][kNStage * kQTileBytes];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long a_tile0 = ((long)blockIdx.x * kNWaves + wave) * kNTiles;
    const long a_tiles_total = (na + kQTileRows - 1) / kQTileRows;
    const long b_tiles_total = (nb + kQTileRows - 1) / kQTileRows;
    const long t_begin = (long)blockIdx.y * tiles_per_split;
    long t_end = t_begin + tiles_per_split;
    t_end = t_end < b_tiles_total ? t_end : b_tiles_total;

    // a tiles of this wave that exist: the others are skipped whole (wave-uniform; every wave still takes part in the
    // DMA issues and the barriers)
    const long left = a_tiles_total - a_tile0;
    const int n_live = left < 0 ? 0 : (left < kNTiles ? (int)left : kNTiles);
    // a fragments: B operand of the MFMA, lane (r, h) holds the bytes 32 s + 16 h .. + 15 of a column's row
    i32x4 af[kNTiles][4];
    unsigned lo_x[kNTiles], hi_x[kNTiles];
#pragma unroll
    for (int q = 0; q < kNTiles; ++q) {
        const long at = a_tile0 + q < a_tiles_total ? a_tile0 + q : a_tiles_total - 1;   // idle tiles load the last one, unused
        long arow = at * kQTileRows + r;
        const bool live = arow < na;
        arow = live ? arow : na - 1;                                                     // idle rows redo the last one
        const unsigned char *src = a + arow * 128 + 16 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) af[q][s] = *reinterpret_cast<const i32x4 *>(src + 32 * s) ^ kSignBits;
        lo_x[q] = excl_lo && live ? excl_lo[arow] : 0u;
        hi_x[q] = excl_lo && live ? excl_hi[arow] : 0u;
    }
    int l_score[kNTiles][K], l_row[kNTiles][K];   // this lane's K best so far, descending; INT_MIN / -1: none
#pragma unroll
    for (int q = 0; q < kNTiles; ++q)
#pragma unroll
        for (int c = 0; c < K; ++c) { l_score[q][c] = INT_MIN; l_row[q][c] = -1; }

    // tiles t .. t + kNStage - 1 of b -> LDS buffer `buf`.  Slot u * kNThreads + threadIdx.x of the stage's 1024 16-byte slots
    // is (tile, chunk c, row rr) in that order; a row beyond nb reads the last row instead (masked in the epilogue)
    auto issue = [&](long t, int buf) {
#pragma unroll
        for (int u = 0; u < kNPieces; ++u) {
            const int slot = u * kNThreads + (int)threadIdx.x;
            const int tile = slot >> 8, c = (slot >> 5) & 7, rr = slot & 31;
            long row = (t + tile) * kQTileRows + rr;
            row = row < nb ? row : nb - 1;
            q8_lds_dma16(b + row * 128 + 16 * c, &s_b[buf][0] + u * (kNThreads * 16) + wave * 1024);
        }
    };
    if (t_begin < t_end) issue(t_begin, 0);
    for (long t0 = t_begin; t0 < t_end; t0 += kNStage) {
        const int buf = (int)(((t0 - t_begin) / kNStage) & 1);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces of the stage have landed
        __syncthreads();                      // ... and everybody's; everybody is also done with the other buffer
        if (t0 + kNStage < t_end) issue(t0 + kNStage, buf ^ 1);
#pragma unroll
        for (int u = 0; u < kNStage; ++u) {
            const long t = t0 + u;
            if (t >= t_end || n_live == 0) break;
            const unsigned char *bb = &s_b[buf][0] + u * kQTileBytes + (h * 32 + r) * 16;
            i32x4 bf[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) bf[s] = *reinterpret_cast<const i32x4 *>(bb + s * 1024) ^ kSignBits;
            const unsigned tile_row0 = (unsigned)(t * kQTileRows);
            const int row0 = (int)tile_row0 + 4 * h;
            const bool tail = (t + 1) * kQTileRows > nb;
#pragma unroll
            for (int q = 0; q < kNTiles; ++q) {
                if (q >= n_live) break;
                i32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf[s], af[q][s], acc, 0, 0, 0);
                // rows masked for this a: beyond nb, or inside the a row's own excluded range
                const bool touch = tail || (tile_row0 < hi_x[q] && tile_row0 + kQTileRows > lo_x[q]);
                if (__builtin_amdgcn_ballot_w64(touch)) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const unsigned row = (unsigned)(row0 + (i & 3) + 8 * (i >> 2));
                        if (row >= (unsigned)nb || (row >= lo_x[q] && row < hi_x[q])) acc[i] = INT_MIN;
                    }
                }
                int m = max3i(acc[0], acc[1], acc[2]);
#pragma unroll
                for (int i = 3; i < 15; i += 2) m = max3i(m, acc[i], acc[i + 1]);
                m = max(m, acc[15]);
                if (__builtin_amdgcn_ballot_w64(m >= l_score[q][K - 1] && m != INT_MIN)) {   // rare once the scan is under way
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int v = acc[i];
                        const bool enters = v >= l_score[q][K - 1] && v != INT_MIN;
                        if (__builtin_amdgcn_ballot_w64(enters))
                            knn_insert_ascending<K>(l_score[q], l_row[q], v, row0 + (i & 3) + 8 * (i >> 2), enters);
                    }
                }
            }
        }
    }
    // fold the two lane halves' row sets (lanes l and l ^ 32 hold the same a column): max-merge the partner's list
#pragma unroll
    for (int q = 0; q < kNTiles; ++q) {
        unsigned long long list[K], other[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            list[c] = l_row[q][c] >= 0 ? knn_key(l_score[q][c], (unsigned)l_row[q][c]) : 0ull;
            const int os = __shfl_xor(l_score[q][c], 32), orow = __shfl_xor(l_row[q][c], 32);
            other[c] = orow >= 0 ? knn_key(os, (unsigned)orow) : 0ull;
        }
#pragma unroll
        for (int c = 0; c < K; ++c) knn_insert<K>(list, other[c]);
        const long arow = (a_tile0 + q) * kQTileRows + r;
        if (h == 0 && a_tile0 + q < a_tiles_total && arow < na) {
            if (final) {
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    if (c < k) {
                        index_out[arow * k + c] = knn_key_index(list[c]);
                        if (score_out) score_out[arow * k + c] = knn_key_score(list[c]);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < K; ++c)
                    if (c < k) part[((long)blockIdx.y * k + c) * na + arow] = list[c];
            }
        }
    }
}

// per a row: the k largest keys of the splits' lists, in ascending split order.  A split's list is descending, so it is left
// at its first key that does not enter.
template <int K>
__global__ __launch_bounds__(256) void knn_q8_merge(const unsigned long long *__restrict__ part, long na, int splits, int k,
                                                     int *__restrict__ index_out, int *__restrict__ score_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    unsigned long long list[K];
#pragma unroll
    for (int c = 0; c < K; ++c) list[c] = 0ull;
    for (int s = 0; s < splits; ++s) {
        for (int c = 0; c < k; ++c) {
            const unsigned long long key = part[((long)s * k + c) * na + i];
            if (key <= list[K - 1]) break;
            knn_insert<K>(list, key);
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (c < k) {
            index_out[i * k + c] = knn_key_index(list[c]);
            if (score_out) score_out[i * k + c] = knn_key_score(list[c]);
        }
    }
}

// The grid and the scratch of a call (lf_mkd_knn_q8_plan is this function; launch_knn_q8 calls it too): match_q8_plan's rule
// at this kernel's block size.
//   a blocks: kNBlockRows rows each.
//   splits:   1 when all of b is one LDS stage (nb <= 128); otherwise about two workgroups per CU in flight, at least 2 and at
//             most one per b tile (and kNMaxSplits) -- a condition on nb alone, so that for a given b the scratch never falls
//             back to 0 as a grows.  No split is empty.
//   scratch:  8 k bytes per (split, a row), stated as  8 k * kNBlockRows * min(A + max(W, A), A * b tiles),  W = 2 * CUs,
//             A = a blocks: an upper bound of splits * na (A * ceil(W / A) < W + A and 2 A <= A + max(W, A)) that is
//             non-decreasing in na, and 0 exactly when splits == 1.
KnnQ8Plan knn_q8_plan(long na, long nb, int k, int num_cus) {
    KnnQ8Plan p{0, 1, 0, 0};
    if (na <= 0) return p;
    const long a_blocks = (na + kNBlockRows - 1) / kNBlockRows;
    const long b_tiles = (nb + kQTileRows - 1) / kQTileRows;
    const long w = 2L * (num_cus > 0 ? num_cus : 256);
    long splits = 1, per = b_tiles;
    if (b_tiles > kNStage) {
        long want = (w + a_blocks - 1) / a_blocks;
        want = want < 2 ? 2 : want;
        want = want > kNMaxSplits ? kNMaxSplits : want;
        want = want > b_tiles ? b_tiles : want;
        per = (b_tiles + want - 1) / want;
        splits = (b_tiles + per - 1) / per;      // no empty split; >= 2 since per < b_tiles
    }
    p.a_blocks = (unsigned)a_blocks;
    p.splits = (unsigned)splits;
    p.tiles_per_split = per;
    if (splits > 1) {
        const long cap = a_blocks + (w > a_blocks ? w : a_blocks);
        const long all = a_blocks * b_tiles;
        p.scratch_bytes = 8ull * (unsigned)k * kNBlockRows * (unsigned long long)(cap < all ? cap : all);
    }
    return p;
}

unsigned knn_q8_block_rows() { return kNBlockRows; }

namespace {
template <int K>
void launch_knn_q8_k(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *excl_lo,
                     const unsigned *excl_hi, int k, const KnnQ8Plan &plan, unsigned long long *part, int *index, int *score,
                     hipStream_t stream) {
    const int splits = (int)plan.splits;
    hipLaunchKernelGGL(knn_q8_scan<K>, dim3(plan.a_blocks, plan.splits), dim3(kNThreads), 0, stream, a, na, b, nb,
                       plan.tiles_per_split, excl_lo, excl_hi, part, splits == 1 ? 1 : 0, k, index, score);
    if (splits > 1)
        hipLaunchKernelGGL(knn_q8_merge<K>, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, stream,
                           (const unsigned long long *)part, na, splits, k, index, score);
}
}  // namespace

void launch_knn_q8(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *excl_lo,
                   const unsigned *excl_hi, int k, const KnnQ8Plan &plan, void *scratch, int *index, int *score,
                   hipStream_t stream) {
    if (na <= 0) return;
    unsigned long long *part = static_cast<unsigned long long *>(scratch);
    if (k <= 2) launch_knn_q8_k<2>(a, na, b, nb, excl_lo, excl_hi, k, plan, part, index, score, stream);
    else if (k <= 4) launch_knn_q8_k<4>(a, na, b, nb, excl_lo, excl_hi, k, plan, part, index, score, stream);
    else if (k <= 8) launch_knn_q8_k<8>(a, na, b, nb, excl_lo, excl_hi, k, plan, part, index, score, stream);
    else launch_knn_q8_k<16>(a, na, b, nb, excl_lo, excl_hi, k, plan, part, index, score, stream);
}

}  // namespace lfmkd
