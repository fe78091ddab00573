// The batched int8 matchers' shared text: what match_q8_pairs (mkd_match_q8.hip), match_q8_edges (mkd_match_q8_edges.hip) and
// match_q8_guided_pairs (mkd_match_q8_guided.hip) have in common beyond the kP* shape of mkd_match_q8_common.h.  A kernel is a
// PROLOGUE (which slot of the grid this workgroup is: q8_pairs_slot over a pair layout, q8_edges_slot over an edge layout and
// two pools) and a BODY over x [nx][128] against y [ny][128] (q8_pairs_block here, q8_guided_block in the guided unit, built
// from the same stage issue, tile update and lane-half fold).  Each unit compiles its own copy, no device code crosses a
// translation unit.  The notes on the form are above match_q8_pairs; DESIGN.md 6f, 6g, 6j.
#pragma once
#include "mkd_match_small.h"       // pair_rows, image_rows, last_pair_at_or_before
#include "mkd_match_q8_common.h"

namespace lfmkd {
namespace {

// What a workgroup of the grid is: block `block` of the x side of pair (edge) p.  x is rows [x_lo, x_lo + nx) of its array and
// y rows [y_lo, y_lo + ny) of the other; the outputs of x row i are entry out_lo + i.  The slot functions fill
// it and return whether the slot has work: false is an idle slot -- in front of the first pair or beyond its pair's rows --,
// nothing to do and nothing of this to be used.
struct Q8Slot {
    long x_lo, nx, y_lo, ny, out_lo, block;
    unsigned p;
    int rev;                                                     // 0: x = a, y = b; 1: the reverse direction, x = b, y = a
};                                                               // (an int: as a bool the guided kernel takes 124 VGPRs, not 122)

// The slot map over a pair layout: the same for the whole workgroup (scalar loads, no divergence).  The outputs are indexed
// like the x rows.
__device__ __forceinline__ bool q8_pairs_slot(const uint64_t *off_a, uint64_t na_total, const uint64_t *off_b, uint64_t nb_total,
                                              unsigned n_pairs, unsigned slots_ab, Q8Slot &s) {
    s.rev = blockIdx.x >= slots_ab;
    const uint64_t slot = s.rev ? blockIdx.x - slots_ab : blockIdx.x;
    const uint64_t *off_x = s.rev ? off_b : off_a, *off_y = s.rev ? off_a : off_b;
    const uint64_t x_total = s.rev ? nb_total : na_total, y_total = s.rev ? na_total : nb_total;
    auto start = [&](unsigned p) { return (off_x[p] < x_total ? off_x[p] : x_total) / kPRows + p; };
    s.p = last_pair_at_or_before(n_pairs, slot, start);
    uint64_t x0 = off_x[s.p], x1 = off_x[s.p + 1], y0 = off_y[s.p], y1 = off_y[s.p + 1];
    asm volatile("" : "+s"(x0), "+s"(x1), "+s"(y0), "+s"(y1));   // (requested together: see match_small_pairs)
    pair_rows(x0, x1, x_total, s.x_lo, s.nx);
    pair_rows(y0, y1, y_total, s.y_lo, s.ny);
    s.out_lo = s.x_lo;
    s.block = (long)slot - (s.x_lo / kPRows + (long)s.p);        // slot - start(p)
    if (s.block < 0) return false;                               // rows in front of the first pair
    return s.block * kPRows < s.nx;                              // (not: the pair's idle slot(s))
}

// The slot map over an EDGE LAYOUT and two pools.  What differs from the pair layout:
//   * the slot map runs over the edge layout of the x side against its capacity -- the same R, the same map, so the grid is
//     what lf_mkd_match_q8_pairs_plan reports for (ea_capacity, eb_capacity, n_edges);
//   * the outputs' base is the edge's first entry of the layout;
//   * x and y are the edge's two IMAGES, taken from the pools through its two ids; y is always the whole image;
//   * the rows served are nx = min(the x image's rows, the edge's range of the layout): entries of the range beyond the image
//     (a layout that was not made from these ids) are left alone, rows of the image beyond the range are not decided;
//   * the body's clamps are therefore to the IMAGE, as the pairs kernel's are to the pair: a DMA lane beyond the image's last
//     row reads the image's last row, an idle x row redoes the image's last served row.  No byte of another image, of the rows
//     that belong to no image, or at or beyond a pool's total is ever requested; no entry at or beyond a capacity is written.
__device__ __forceinline__ bool q8_edges_slot(const uint64_t *image_off_a, unsigned n_images_a, uint64_t na_total,
                                                const uint64_t *image_off_b, unsigned n_images_b, uint64_t nb_total,
                                                const unsigned *edge_a, const unsigned *edge_b, const uint64_t *edge_off_a,
                                                uint64_t ea_capacity, const uint64_t *edge_off_b, uint64_t eb_capacity,
                                                unsigned n_edges, unsigned slots_ab, Q8Slot &s) {
    s.rev = blockIdx.x >= slots_ab;
    const uint64_t slot = s.rev ? blockIdx.x - slots_ab : blockIdx.x;
    const uint64_t *off_x = s.rev ? edge_off_b : edge_off_a;
    const uint64_t x_capacity = s.rev ? eb_capacity : ea_capacity;
    auto start = [&](unsigned p) { return (off_x[p] < x_capacity ? off_x[p] : x_capacity) / kPRows + p; };
    s.p = last_pair_at_or_before(n_edges, slot, start);
    long len;
    pair_rows(off_x[s.p], off_x[s.p + 1], x_capacity, s.out_lo, len);
    s.block = (long)slot - (s.out_lo / kPRows + (long)s.p);      // slot - start(p)
    if (s.block < 0) return false;                               // entries in front of the first edge
    // (requesting the two ids together with the offsets above, and the four image offsets in one round trip behind them,
    //  was measured against this form in one run, alternating: 256 frames with window 4 at 1.010 .. 1.019 x the pairs call
    //  against 1.013 .. 1.025 x -- not resolved, so the plain form stays)
    const unsigned id_a = edge_a[s.p], id_b = edge_b[s.p];
    long a_lo, a_n, b_lo, b_n;
    image_rows(image_off_a, n_images_a, na_total, id_a, a_lo, a_n);
    image_rows(image_off_b, n_images_b, nb_total, id_b, b_lo, b_n);
    s.x_lo = s.rev ? b_lo : a_lo;
    s.y_lo = s.rev ? a_lo : b_lo;
    s.ny = s.rev ? a_n : b_n;
    s.nx = s.rev ? b_n : a_n;
    s.nx = s.nx < len ? s.nx : len;                              // the rows served
    return s.block * kPRows < s.nx;                              // (not: the edge's idle slot(s))
}

// no candidate for any row of the block: -1 / INT32_MIN / INT32_MIN
__device__ __forceinline__ void q8_fill_none(int *match, int *best_o, int *second_o, long block, long nx) {
    for (long row = block * kPRows + threadIdx.x; row < nx && row < (block + 1) * kPRows; row += kPThreads) {
        match[row] = -1;
        if (best_o) best_o[row] = INT_MIN;
        if (second_o) second_o[row] = INT_MIN;
    }
}

// tiles t .. t + kPStage - 1 of y -> the LDS stage at dst.  Slot u * kPThreads + threadIdx.x of the stage's 16-byte slots is
// (tile, chunk c, row rr) in that order; a row beyond ny reads the last y row instead (masked in the epilogue)
__device__ __forceinline__ void q8_issue_stage(const unsigned char *y, long ny, long t, unsigned char *dst, int wave) {
#pragma unroll
    for (int u = 0; u < kPPieces; ++u) {
        const int sl = u * kPThreads + (int)threadIdx.x;
        const int tile = sl >> 8, c = (sl >> 5) & 7, rr = sl & 31;
        long row = (t + tile) * kQTileRows + rr;
        row = row < ny ? row : ny - 1;
        q8_lds_dma16(y + row * 128 + 16 * c, dst + u * (kPThreads * 16) + wave * 1024);
    }
}

// a finished 32 x 32 tile into the lane's running best / second / index: the lane's 16 y rows are row0 + (i & 3) + 8 (i >> 2),
// masked sums are INT32_MIN.  (acc by value: by reference match_q8_pairs takes 86 VGPRs, not 84)
__device__ __forceinline__ void q8_take_tile(i32x16 acc, int row0, int &best, int &second, int &best_i) {
    int m = max3i(acc[0], acc[1], acc[2]);
#pragma unroll
    for (int i = 3; i < 15; i += 2) m = max3i(m, acc[i], acc[i + 1]);
    m = max(m, acc[15]);
    if (__builtin_amdgcn_ballot_w64(m > second || m >= best)) {   // rare once the scan is under way
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int v = acc[i];
            const int row = row0 + (i & 3) + 8 * (i >> 2);
            const bool nb_ = v >= best && v != INT_MIN;   // later index wins among equals
            const bool ns = !nb_ && v > second;
            second = nb_ ? best : (ns ? v : second);
            best_i = nb_ ? row : best_i;
            best = nb_ ? v : best;
        }
    }
}

// fold the two lane halves' row sets (lanes l and l ^ 32 hold the same x column)
struct Q8Top {
    int best, second, index;
};
__device__ __forceinline__ Q8Top q8_fold_halves(int best, int second, int best_i) {
    const int ob = __shfl_xor(best, 32), os = __shfl_xor(second, 32), oi = __shfl_xor(best_i, 32);
    // (| and &, and the result by value: with || and && and reference outputs this becomes three branches behind the stage
    //  loop where the kernels had selects)
    const bool other = (ob > best) | ((ob == best) & (oi > best_i));
    return {other ? ob : best, other ? max(best, os) : max(second, ob), other ? oi : best_i};
}

// The plain body of a workgroup: x [nx][128] against y [ny][128] is the whole problem, nx >= 1, ny >= 2 -- a pair's rows or an
// edge's two images, so every clamp below is to what the prologue handed over and to nothing else.  s_y: the kernel's two LDS
// stages.
__device__ __forceinline__ void q8_pairs_block(const unsigned char *__restrict__ x, long nx,
                                               const unsigned char *__restrict__ y, long ny, float ratio,
                                               int *__restrict__ match, int *__restrict__ best_o, int *__restrict__ second_o,
                                               long block, unsigned char (&s_y)[2][kPStage * kQTileBytes]) {
    __builtin_assume(nx >= 1);   // (a slot with work; said here because the slot function's own tests do not reach the divisions below)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long x_tile0 = (block * kPWaves + wave) * kPTiles;
    const long x_tiles_total = (nx + kQTileRows - 1) / kQTileRows;
    const long y_tiles_total = (ny + kQTileRows - 1) / kQTileRows;
    // x tiles of this wave that exist: the others are skipped whole (wave-uniform; every wave still takes part in the DMA
    // issues and the barriers)
    const long left = x_tiles_total - x_tile0;
    const int n_live = left < 0 ? 0 : (left < kPTiles ? (int)left : kPTiles);
    // x fragments: B operand of the MFMA, lane (r, h) holds the bytes 32 s + 16 h .. + 15 of a column's row
    i32x4 xf[kPTiles][4];
#pragma unroll
    for (int q = 0; q < kPTiles; ++q) {
        const long xt = x_tile0 + q < x_tiles_total ? x_tile0 + q : x_tiles_total - 1;   // idle tiles load the last one, unused
        long xrow = xt * kQTileRows + r;
        xrow = xrow < nx ? xrow : nx - 1;                                                // idle rows redo the last x row
        const unsigned char *src = x + xrow * 128 + 16 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) xf[q][s] = *reinterpret_cast<const i32x4 *>(src + 32 * s) ^ kSignBits;
    }
    int best[kPTiles], second[kPTiles], best_i[kPTiles];
#pragma unroll
    for (int q = 0; q < kPTiles; ++q) { best[q] = INT_MIN; second[q] = INT_MIN; best_i[q] = -1; }

    q8_issue_stage(y, ny, 0, &s_y[0][0], wave);
    for (long t0 = 0; t0 < y_tiles_total; t0 += kPStage) {
        const int buf = (int)((t0 / kPStage) & 1);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces of the stage have landed
        __syncthreads();                      // ... and everybody's; everybody is also done with the other buffer
        if (t0 + kPStage < y_tiles_total) q8_issue_stage(y, ny, t0 + kPStage, &s_y[buf ^ 1][0], wave);
#pragma unroll
        for (int u = 0; u < kPStage; ++u) {
            const long t = t0 + u;
            if (t >= y_tiles_total || n_live == 0) break;
            const unsigned char *yy = &s_y[buf][0] + u * kQTileBytes + (h * 32 + r) * 16;
            i32x4 yf[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) yf[s] = *reinterpret_cast<const i32x4 *>(yy + s * 1024) ^ kSignBits;
            const int row0 = (int)(t * kQTileRows) + 4 * h;
            const bool tail = (t + 1) * kQTileRows > ny;
            // the wave's x tiles.  (do-while: with kPTiles == 1 this is no loop.  Round a `for` the 16 row numbers of
            // q8_take_tile, which do not depend on q, are lifted out of it as loop invariants and so out of its rare branch:
            // 14 64-bit additions per tile in front of the matrix instructions of EVERY tile)
            int q = 0;
#pragma unroll
            do {
                if (q >= n_live) break;
                i32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(yf[s], xf[q][s], acc, 0, 0, 0);
                if (tail) {                   // rows beyond the last y row (wave-uniform)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (row0 + (i & 3) + 8 * (i >> 2) >= ny) acc[i] = INT_MIN;
                }
                q8_take_tile(acc, row0, best[q], second[q], best_i[q]);
            } while (++q < kPTiles);
        }
    }
#pragma unroll
    for (int q = 0; q < kPTiles; ++q) {
        const Q8Top top = q8_fold_halves(best[q], second[q], best_i[q]);
        const int nbest = top.best, nsecond = top.second, nidx = top.index;
        const long xrow = (x_tile0 + q) * kQTileRows + r;
        if (h == 0 && q < n_live && xrow < nx) {
            match[xrow] = q8_decide(nbest, nidx, nsecond, ratio);
            if (best_o) best_o[xrow] = nbest;
            if (second_o) second_o[xrow] = nsecond;
        }
    }
}

}  // namespace
}  // namespace lfmkd
