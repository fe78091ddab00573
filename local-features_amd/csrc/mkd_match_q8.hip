// gfx950 8-bit descriptors: the quantiser and the exact int8 matcher (include/lf_mkd.h, "8-bit descriptors").
//
// A quantised row is 128 offset-binary bytes, byte = q + 128 with q in [-127, 127].  The similarity of two rows is the exact
// integer  sum_k q_a[k] q_b[k]  (|.| <= 128 * 127^2 < 2^24), so the matcher has ONE form: no margin, no re-score, no
// fallback.  It is `match_scan` of mkd_match.hip with the operands changed:
//
//   * v_mfma_i32_32x32x32_i8, b on the M side: 4 matrix instructions per 32 x 32 tile of pairs (K = 128).  A lane of an
//     accumulator tile holds ONE a column and 16 b rows; the running best / second of an a row is an in-register reduction.
//   * a fragments: lane (r = lane & 31, h = lane >> 5) keeps the 16 bytes at offset 32 s + 16 h of its row for k-step s,
//     XORed with 0x80808080 once (offset binary -> two's complement): 16 VGPRs per 32-row tile, kQTiles tiles per wave.
//   * b needs no pre-tiling pass: the LDS-DMA takes a per-lane GLOBAL address and writes LDS lane-contiguously, so the lane
//     that fills LDS slot (16-byte chunk c, row r) of a tile's [chunk 8][row 32][16 B] image fetches
//     b + (row0 + r) * 128 + 16 c.  A fragment read is then one ds_read_b128 over 1 KiB of consecutive bytes per wave
//     (conflict-free); the b fragment is XORed after the read.  kQStage tiles per barrier, double buffered.
//   * the k order inside an i8 fragment need not be known: both operands are fetched by the same (lane half, chunk) rule and
//     integer addition is exact, so any consistent permutation of k gives the same sum.
//
// Grid = (a blocks of kQBlockRows rows, b splits).  With one split the scan writes the final result itself; otherwise it
// writes partial (best, index, second) per (split, a row) and `match_q8_merge` folds them in ascending b order and applies
// the acceptance rule.  Masked candidates (beyond nb, or inside the a row's excluded range) are INT32_MIN, below every sum.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_match_q8_batched.h"  // match_q8_pairs' slot map and body; through it mkd_match_q8_common.h: the tile constants,
                                   // q8_lds_dma16, max3i, q8_decide, the batched form's kP* shape

namespace lfmkd {
namespace {

constexpr int kQWaves = 8, kQTiles = 4;            // per wave: 4 a tiles = 64 VGPRs of fragments
constexpr int kQStage = 4;                         // b tiles per LDS stage: 16 KiB = 512 threads x 2 x 16 B
constexpr int kQBlockRows = kQWaves * kQTiles * kQTileRows;
constexpr int kQMaxSplits = 1024;

}  // namespace

// x [n][128] f32 -> q [n][128] bytes: a thread converts 4 floats into one dword
__global__ __launch_bounds__(256) void quantize_rows(const float4 *__restrict__ x, unsigned long long n4, float scale,
                                                     unsigned *__restrict__ q) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = x[i];
    const float e[4] = {v.x, v.y, v.z, v.w};
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float p = rintf(e[j] * scale);                                  // ties to even (v_rndne_f32)
        const float c = p != p ? 0.f : fminf(fmaxf(p, -127.f), 127.f);        // NaN -> 0, +-inf saturate
        w |= (unsigned)((int)c + 128) << (8 * j);
    }
    q[i] = w;
}

// final != 0 (one split): match / best_out / second_out are written here and the p_* are not used
__global__ __launch_bounds__(512) void match_q8_scan(const unsigned char *__restrict__ a, long na,
                                                     const unsigned char *__restrict__ b, long nb, long tiles_per_split,
                                                     const unsigned *__restrict__ excl_lo,
                                                     const unsigned *__restrict__ excl_hi, int *__restrict__ p_best,
                                                     int *__restrict__ p_index, int *__restrict__ p_second, int final,
                                                     float ratio, int *__restrict__ match, int *__restrict__ best_out,
                                                     int *__restrict__ second_out) {
    __shared__ __attribute__((aligned(16))) unsigned char s_b[2][kQStage * kQTileBytes];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long a_tile0 = ((long)blockIdx.x * kQWaves + wave) * kQTiles;
    const long a_tiles_total = (na + kQTileRows - 1) / kQTileRows;
    const long b_tiles_total = (nb + kQTileRows - 1) / kQTileRows;
    const long t_begin = (long)blockIdx.y * tiles_per_split;
    long t_end = t_begin + tiles_per_split;
    t_end = t_end < b_tiles_total ? t_end : b_tiles_total;

    // a tiles of this wave that exist: the others are skipped whole (wave-uniform; every wave still takes part in the
    // DMA issues and the barriers)
    const long left = a_tiles_total - a_tile0;
    const int n_live = left < 0 ? 0 : (left < kQTiles ? (int)left : kQTiles);
    // a fragments: B operand of the MFMA, lane (r, h) holds the bytes 32 s + 16 h .. + 15 of a column's row
    i32x4 af[kQTiles][4];
    unsigned lo_x[kQTiles], hi_x[kQTiles];
#pragma unroll
    for (int q = 0; q < kQTiles; ++q) {
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
    int best[kQTiles], second[kQTiles], best_i[kQTiles];
#pragma unroll
    for (int q = 0; q < kQTiles; ++q) { best[q] = INT_MIN; second[q] = INT_MIN; best_i[q] = -1; }

    // tiles t .. t + kQStage - 1 of b -> LDS buffer `buf`.  Slot u * 512 + threadIdx.x of the stage's 1024 16-byte slots is
    // (tile, chunk c, row rr) in that order; a row beyond nb reads the last row instead (masked in the epilogue)
    auto issue = [&](long t, int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int slot = u * 512 + (int)threadIdx.x;
            const int tile = slot >> 8, c = (slot >> 5) & 7, rr = slot & 31;
            long row = (t + tile) * kQTileRows + rr;
            row = row < nb ? row : nb - 1;
            q8_lds_dma16(b + row * 128 + 16 * c, &s_b[buf][0] + u * 8192 + wave * 1024);
        }
    };
    if (t_begin < t_end) issue(t_begin, 0);
    for (long t0 = t_begin; t0 < t_end; t0 += kQStage) {
        const int buf = (int)(((t0 - t_begin) / kQStage) & 1);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces of the stage have landed
        __syncthreads();                      // ... and everybody's; everybody is also done with the other buffer
        if (t0 + kQStage < t_end) issue(t0 + kQStage, buf ^ 1);
#pragma unroll
        for (int u = 0; u < kQStage; ++u) {
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
            for (int q = 0; q < kQTiles; ++q) {
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
                if (__builtin_amdgcn_ballot_w64(m > second[q] || m >= best[q])) {   // rare once the scan is under way
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int v = acc[i];
                        const int row = row0 + (i & 3) + 8 * (i >> 2);
                        const bool nb_ = v >= best[q] && v != INT_MIN;   // later index wins among equals
                        const bool ns = !nb_ && v > second[q];
                        second[q] = nb_ ? best[q] : (ns ? v : second[q]);
                        best_i[q] = nb_ ? row : best_i[q];
                        best[q] = nb_ ? v : best[q];
                    }
                }
            }
        }
    }
    // fold the two lane halves' row sets (lanes l and l ^ 32 hold the same a column)
#pragma unroll
    for (int q = 0; q < kQTiles; ++q) {
        const int ob = __shfl_xor(best[q], 32), os = __shfl_xor(second[q], 32), oi = __shfl_xor(best_i[q], 32);
        const bool other = ob > best[q] || (ob == best[q] && oi > best_i[q]);
        const int nbest = other ? ob : best[q];
        const int nsecond = other ? max(best[q], os) : max(second[q], ob);
        const int nidx = other ? oi : best_i[q];
        const long arow = (a_tile0 + q) * kQTileRows + r;
        if (h == 0 && a_tile0 + q < a_tiles_total && arow < na) {
            if (final) {
                match[arow] = q8_decide(nbest, nidx, nsecond, ratio);
                if (best_out) best_out[arow] = nbest;
                if (second_out) second_out[arow] = nsecond;
            } else {
                const long o = (long)blockIdx.y * na + arow;
                p_best[o] = nbest;
                p_index[o] = nidx;
                p_second[o] = nsecond;
            }
        }
    }
}

// folds the splits of one a row in ascending b order (the later range wins among equals) and applies the acceptance rule
__global__ __launch_bounds__(256) void match_q8_merge(const int *__restrict__ p_best, const int *__restrict__ p_index,
                                                      const int *__restrict__ p_second, long na, int splits, float ratio,
                                                      int *__restrict__ match, int *__restrict__ best_out,
                                                      int *__restrict__ second_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    int b = INT_MIN, s = INT_MIN, bi = -1;
    for (int k = 0; k < splits; ++k) {
        const int ob = p_best[(long)k * na + i], os = p_second[(long)k * na + i], oi = p_index[(long)k * na + i];
        const bool other = oi >= 0 && ob >= b;
        s = other ? max(b, os) : max(s, ob);
        bi = other ? oi : bi;
        b = other ? ob : b;
    }
    match[i] = q8_decide(b, bi, s, ratio);
    if (best_out) best_out[i] = b;
    if (second_out) second_out[i] = s;
}

// ---- many pairs in ONE launch (lf_mkd_match_q8_pairs_device) -------------------------------------------------
// The layout of lf_mkd_match_pairs_device over u8 rows: pair p is rows [off_a[p], off_a[p + 1]) of a against rows
// [off_b[p], off_b[p + 1]) of b, the offsets on the device and never read by the host.  The grid is sized from the totals
// alone with match_small_pairs' slot map at block size R = kPRows instead of 16: pair p owns the slots from
// floor(min(off[p], total) / R) + p on.  That start is strictly increasing in p (the offsets are non-decreasing), and the next
// pair's start is at least ceil(n_p / R) further on, because  ceil(n / R) <= floor((o + n) / R) - floor(o / R) + 1  for any
// R >= 1 (write o = q R + r, 0 <= r < R: floor((o + n) / R) - q = floor((r + n) / R) >= floor(n / R), and
// ceil(n / R) <= floor(n / R) + 1); the last pair ends at or before floor(n_total / R) + n_pairs, the grid of one direction.
// At most one idle slot per pair and R-th of a row.  With match_ba the slots of b's rows follow those of a's and run the same
// body with the operands' roles exchanged.
//
// A workgroup owns R rows of its pair's x side (kPWaves waves x kPTiles tiles of 32) and sees the WHOLE y side of the pair:
// no splits, no partials, no merge launch.  y is streamed through LDS as match_q8_scan streams b -- the per-lane LDS-DMA into
// the [chunk 8][row 32][16 B] tile image, XOR after the read, kPStage tiles per barrier, double buffered, vmcnt(0) plus a
// barrier per stage -- and every (x row, y row) sum is the same exact integer, so with the same tie rule (the highest index)
// every output equals the single-pair call's on the pair's rows alone.
// The clamps are to the PAIR, not to the array: the body is handed x = the pair's first x row and nx = its row count
// (likewise y, ny), so a DMA lane beyond the pair's last y row reads the pair's last y row (masked to INT32_MIN in the
// epilogue) and an idle x row redoes the pair's last x row.  No byte of another pair, of the rows in front of the first or
// behind the last pair, or at or beyond a total is ever requested.
// (the workgroup's shape -- kPWaves, kPTiles, kPStage, R = kPRows -- is in mkd_match_q8_common.h; the slot map, q8_pairs_slot,
// and the body, q8_pairs_block, are in mkd_match_q8_batched.h, where the edges and the guided form find them too)
__global__ __launch_bounds__(kPThreads) void match_q8_pairs(const unsigned char *__restrict__ a,
                                                            const uint64_t *__restrict__ off_a, uint64_t na_total,
                                                            const unsigned char *__restrict__ b,
                                                            const uint64_t *__restrict__ off_b, uint64_t nb_total,
                                                            unsigned n_pairs, unsigned slots_ab, float ratio,
                                                            int *__restrict__ match_ab, int *__restrict__ match_ba,
                                                            int *__restrict__ best_out, int *__restrict__ second_out) {
    __shared__ __attribute__((aligned(16))) unsigned char s_y[2][kPStage * kQTileBytes];
    Q8Slot s;
    if (!q8_pairs_slot(off_a, na_total, off_b, nb_total, n_pairs, slots_ab, s)) return;   // an idle slot
    int *match = (s.rev ? match_ba : match_ab) + s.out_lo;
    int *best_o = s.rev || !best_out ? nullptr : best_out + s.out_lo;
    int *second_o = s.rev || !second_out ? nullptr : second_out + s.out_lo;
    if (s.ny < 2) {                                              // a side the single-pair call refuses
        q8_fill_none(match, best_o, second_o, s.block, s.nx);
        return;
    }
    // from here on the pair is the whole problem: x [nx][128] against y [ny][128]
    const unsigned char *x = (s.rev ? b : a) + s.x_lo * 128, *y = (s.rev ? a : b) + s.y_lo * 128;
    q8_pairs_block(x, s.nx, y, s.ny, ratio, match, best_o, second_o, s.block, s_y);
}

// The grid and the scratch of a call (lf_mkd_match_q8_plan is this function; launch_match_q8 calls it too).
//   a blocks: kQBlockRows rows each.
//   splits:   1 when all of b is one LDS stage (nb <= 128: nothing to share out); otherwise about two workgroups per CU
//             in flight, at least 2 and at most one per b tile -- a condition on nb alone, so that for a given b the
//             scratch never falls back to 0 as a grows.  (Two splits where one would do, at 2^20 x 2^20, cost one merge
//             launch over 24 MiB beside a scan of 2^40 pairs.)
//   scratch:  12 bytes per (split, a row), stated as  12 * kQBlockRows * min(A + max(W, A), A * b tiles),  W = 2 * CUs,
//             A = a blocks: an upper bound of splits * na (A * ceil(W / A) < W + A and 2 A <= A + max(W, A)) that is
//             non-decreasing in na, within 2x of it, and 0 exactly when splits == 1.
Q8Plan match_q8_plan(long na, long nb, int num_cus) {
    Q8Plan p{0, 1, 0, 0};
    if (na <= 0) return p;
    const long a_blocks = (na + kQBlockRows - 1) / kQBlockRows;
    const long b_tiles = (nb + kQTileRows - 1) / kQTileRows;
    const long w = 2L * (num_cus > 0 ? num_cus : 256);
    long splits = 1, per = b_tiles;
    if (b_tiles > kQStage) {
        long want = (w + a_blocks - 1) / a_blocks;
        want = want < 2 ? 2 : want;
        want = want > kQMaxSplits ? kQMaxSplits : want;
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
        p.scratch_bytes = 12ull * kQBlockRows * (unsigned long long)(cap < all ? cap : all);
    }
    return p;
}

void launch_quantize_rows(const float *x, unsigned long long n, float scale, unsigned char *q, hipStream_t stream) {
    if (n == 0) return;
    const unsigned long long n4 = n * 32;
    hipLaunchKernelGGL(quantize_rows, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const float4 *>(x), n4, scale, reinterpret_cast<unsigned *>(q));
}

void launch_match_q8(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *excl_lo,
                     const unsigned *excl_hi, float ratio, const Q8Plan &plan, void *scratch, int *match, int *best,
                     int *second, hipStream_t stream) {
    if (na <= 0) return;
    const int splits = (int)plan.splits;
    int *p_best = static_cast<int *>(scratch);
    int *p_second = p_best ? p_best + (size_t)splits * na : nullptr;
    int *p_index = p_best ? p_second + (size_t)splits * na : nullptr;
    hipLaunchKernelGGL(match_q8_scan, dim3(plan.a_blocks, plan.splits), dim3(512), 0, stream, a, na, b, nb,
                       plan.tiles_per_split, excl_lo, excl_hi, p_best, p_index, p_second, splits == 1 ? 1 : 0, ratio, match,
                       best, second);
    if (splits > 1)
        hipLaunchKernelGGL(match_q8_merge, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, stream, (const int *)p_best,
                           (const int *)p_index, (const int *)p_second, na, splits, ratio, match, best, second);
}

unsigned match_q8_pairs_block_rows() { return kPRows; }
uint64_t match_q8_pairs_slots(uint64_t n_total, unsigned n_pairs) { return n_total / kPRows + n_pairs; }

void launch_match_q8_pairs(const unsigned char *a, const uint64_t *off_a, uint64_t na_total, const unsigned char *b,
                           const uint64_t *off_b, uint64_t nb_total, unsigned n_pairs, float ratio, bool mutual, int *match_ab,
                           int *match_ba, int *best, int *second, hipStream_t stream) {
    if (n_pairs == 0) return;
    const uint64_t slots_ab = match_q8_pairs_slots(na_total, n_pairs);
    const uint64_t slots = slots_ab + (match_ba ? match_q8_pairs_slots(nb_total, n_pairs) : 0);
    hipLaunchKernelGGL(match_q8_pairs, dim3((unsigned)slots), dim3(kPThreads), 0, stream, a, off_a, na_total, b, off_b,
                       nb_total, n_pairs, (unsigned)slots_ab, ratio, match_ab, match_ba, best, second);
    if (mutual) launch_match_mutual(off_a, na_total, off_b, nb_total, n_pairs, match_ab, match_ba, stream);
}

}  // namespace lfmkd
