// gfx950 grouped matching over 8-bit descriptors: the ratio test against the best neighbour from ANOTHER group, and the
// group-by-group vote table of the matches (include/lf_mkd.h, lf_mkd_match_q8_grouped_device, lf_mkd_vote_groups_device;
// DESIGN.md 6i).
//
// `match_q8_scan` / `knn_q8_scan` with another epilogue.  Everything in front of it is those kernels': the a fragments in
// registers (XORed once), b straight from the caller's rows by per-lane LDS-DMA into the [chunk 8][row 32][16 B] tile image
// (XOR after the read), kGStage tiles per barrier, double buffered, vmcnt(0) plus a barrier per stage, four
// v_mfma_i32_32x32x32_i8 per 32 x 32 tile of pairs, the clamps on the DMA address (nb - 1) and on idle a rows (na - 1), masked
// candidates at INT32_MIN.  No request leaves [0, na) / [0, nb).
//
// The epilogue keeps, per lane and a tile, the state (best, index, group of best, rival): rival is the best score among the
// rows seen whose group differs from the best's.  A candidate is ordered as in the top-k call (larger s first, among equal s
// the higher index first); a lane meets its rows in ascending order, so "in front of the best" is the 32-bit test v >= best.
//   scan   v >= best:  if a best exists and group != best_group, rival = best;  then best, index, best_group = v, row, group
//          else if group != best_group && v > rival:  rival = v
//   merge  W = the state with the larger (best, index), L the other; a state without a candidate is the identity;
//          W with rival = max(W.rival, best groups differ ? L.best : L.rival)
// Each merge yields the definition's value for the union of the two row sets, so the fold of the lane halves, the merge of the
// splits and any order of either give the same answer: not a function of the split count or the CU count.
//
// The update is gated as the top-2 code gates its own: v_max3_i32 over the tile's 16 values, then
// ballot((m > rival || m >= best) && m != INT_MIN).  Group ids are needed only behind that gate.  They are staged with the
// b stage: waves 0 and 1 fetch the stage's 4 x 32 ids by one dword of LDS-DMA per lane under the rows' own clamp (nb - 1), into
// the 512 bytes behind the stage's tile images, and a gated tile reads its lane's 16 ids with four ds_read_b128 (a lane's rows
// are four runs of 4; within a lane half every lane reads the same address).  LF_Q8_GROUPED_STAGED_IDS=0 builds the other
// route, 16 loads per lane from global memory inside the gate; DESIGN.md 6i has both measured.  No request for a group id
// leaves [0, nb).  With a single group nothing ever raises rival and the gate never closes (the header says so).
//
// Grid = (a blocks of kGBlockRows rows, b splits).  With one split the scan writes match / best / rival itself; otherwise it
// writes each row's state for its split (16 bytes) and `match_q8_grouped_merge` folds the splits and applies the acceptance
// rule.  `vote_groups` at the end of the file is the integer scatter that turns matches into a [groups of a][groups of b] table.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_match_q8_common.h"   // the tile constants, q8_lds_dma16, max3i, q8_decide

// the workgroup (8 x 1 measured beside match_q8_scan's 8 x 4)
#ifndef LF_Q8_GROUPED_WAVES
#define LF_Q8_GROUPED_WAVES 8
#endif
#ifndef LF_Q8_GROUPED_TILES
#define LF_Q8_GROUPED_TILES 1
#endif
// where a gated tile takes its 32 group ids from (both measured): 1 = staged with the b stage into LDS,
// 0 = fetched per lane from global memory inside the gate
#ifndef LF_Q8_GROUPED_STAGED_IDS
#define LF_Q8_GROUPED_STAGED_IDS 1
#endif

namespace lfmkd {
namespace {

constexpr int kGWaves = LF_Q8_GROUPED_WAVES, kGTiles = LF_Q8_GROUPED_TILES;
constexpr int kGThreads = 64 * kGWaves;
constexpr int kGStage = 4;                                   // b tiles per LDS stage: 16 KiB
constexpr int kGPieces = kGStage * 256 / kGThreads;          // 16-byte DMA pieces per thread and stage
constexpr int kGBlockRows = kGWaves * kGTiles * kQTileRows;
constexpr int kGMaxSplits = 1024;
constexpr bool kGStagedIds = LF_Q8_GROUPED_STAGED_IDS != 0;
constexpr int kGTilesBytes = kGStage * kQTileBytes;                              // a stage's tile images ...
constexpr int kGStageBytes = kGTilesBytes + (kGStagedIds ? kGStage * 128 : 0);   // ... and behind them its rows' group ids
static_assert(kGPieces * kGThreads == kGStage * 256 && kGPieces >= 1, "whole pieces");
static_assert(kGWaves >= 2, "two waves fetch a stage's 128 group ids");

// a row's running state; index < 0: no candidate yet (best == rival == INT_MIN, group unused)
struct GroupedState {
    int best, index;
    unsigned group;
    int rival;
};

// the merge of two states over disjoint row sets (the file's head)
__device__ __forceinline__ GroupedState grouped_merge(const GroupedState &x, const GroupedState &y) {
    const bool y_wins = y.best > x.best || (y.best == x.best && y.index > x.index);
    const GroupedState w = y_wins ? y : x, l = y_wins ? x : y;
    GroupedState out = w;
    // a loser without a candidate has best == rival == INT_MIN: the identity whatever its group word holds
    out.rival = max(w.rival, w.group != l.group ? l.best : l.rival);
    return out;
}

}  // namespace

// final != 0 (one split): match / best_out / rival_out are written here and part is not used.
// part: [split][na] states as int4 (best, index, group, rival)
__global__ __launch_bounds__(kGThreads) void match_q8_grouped_scan(const unsigned char *__restrict__ a, long na,
                                                                    const unsigned char *__restrict__ b, long nb,
                                                                    long tiles_per_split,
                                                                    const unsigned *__restrict__ group_of_b,
                                                                    const unsigned *__restrict__ excl_lo,
                                                                    const unsigned *__restrict__ excl_hi,
                                                                    int4 *__restrict__ part, int final, float ratio,
                                                                    int *__restrict__ match, int *__restrict__ best_out,
                                                                    int *__restrict__ rival_out) {
    __shared__ __attribute__((aligned(16))) unsigned char s_b[2][kGStageBytes];   // (one array: tiles and ids)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long a_tile0 = ((long)blockIdx.x * kGWaves + wave) * kGTiles;
    const long a_tiles_total = (na + kQTileRows - 1) / kQTileRows;
    const long b_tiles_total = (nb + kQTileRows - 1) / kQTileRows;
    const long t_begin = (long)blockIdx.y * tiles_per_split;
    long t_end = t_begin + tiles_per_split;
    t_end = t_end < b_tiles_total ? t_end : b_tiles_total;

    // a tiles of this wave that exist: the others are skipped whole (wave-uniform; every wave still takes part in the
    // DMA issues and the barriers)
    const long left = a_tiles_total - a_tile0;
    const int n_live = left < 0 ? 0 : (left < kGTiles ? (int)left : kGTiles);
    // a fragments: B operand of the MFMA, lane (r, h) holds the bytes 32 s + 16 h .. + 15 of a column's row
    i32x4 af[kGTiles][4];
    unsigned lo_x[kGTiles], hi_x[kGTiles];
#pragma unroll
    for (int q = 0; q < kGTiles; ++q) {
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
    int best[kGTiles], best_i[kGTiles], rival[kGTiles];
    unsigned best_g[kGTiles];
#pragma unroll
    for (int q = 0; q < kGTiles; ++q) { best[q] = INT_MIN; best_i[q] = -1; best_g[q] = 0u; rival[q] = INT_MIN; }

    // tiles t .. t + kGStage - 1 of b -> LDS buffer `buf`.  Slot u * kGThreads + threadIdx.x of the stage's 1024 16-byte slots
    // is (tile, chunk c, row rr) in that order; a row beyond nb reads the last row instead (masked in the epilogue)
    auto issue = [&](long t, int buf) {
#pragma unroll
        for (int u = 0; u < kGPieces; ++u) {
            const int slot = u * kGThreads + (int)threadIdx.x;
            const int tile = slot >> 8, c = (slot >> 5) & 7, rr = slot & 31;
            long row = (t + tile) * kQTileRows + rr;
            row = row < nb ? row : nb - 1;
            q8_lds_dma16(b + row * 128 + 16 * c, &s_b[buf][0] + u * (kGThreads * 16) + wave * 1024);
        }
        // the stage's 128 group ids, one dword per lane of waves 0 and 1, under the same clamp
        if (kGStagedIds && wave < 2) {
            long row = t * kQTileRows + (long)threadIdx.x;
            row = row < nb ? row : nb - 1;
            q8_lds_dma4(group_of_b + row, &s_b[buf][0] + kGTilesBytes + wave * 256);
        }
    };
    if (t_begin < t_end) issue(t_begin, 0);
    for (long t0 = t_begin; t0 < t_end; t0 += kGStage) {
        const int buf = (int)(((t0 - t_begin) / kGStage) & 1);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces of the stage have landed
        __syncthreads();                      // ... and everybody's; everybody is also done with the other buffer
        if (t0 + kGStage < t_end) issue(t0 + kGStage, buf ^ 1);
#pragma unroll
        for (int u = 0; u < kGStage; ++u) {
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
            for (int q = 0; q < kGTiles; ++q) {
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
                if (__builtin_amdgcn_ballot_w64((m > rival[q] || m >= best[q]) && m != INT_MIN)) {   // rare once the scan is under way
                    // the group ids of this lane's 16 rows, all requested before the first is used: four 16-byte LDS reads
                    // of the staged ids, or 16 loads under the DMA's clamp (a clamped row's value is masked)
                    unsigned gid[16];
                    if (kGStagedIds) {
                        const uint4 *ids = reinterpret_cast<const uint4 *>(&s_b[buf][0] + kGTilesBytes + u * 128 + 16 * h);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint4 w = ids[2 * j];
                            gid[4 * j] = w.x; gid[4 * j + 1] = w.y; gid[4 * j + 2] = w.z; gid[4 * j + 3] = w.w;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const long row = (long)row0 + (i & 3) + 8 * (i >> 2);
                            gid[i] = group_of_b[row < nb ? row : nb - 1];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int v = acc[i];
                        const int row = row0 + (i & 3) + 8 * (i >> 2);
                        // a value that can change the state (never a masked one)
                        const bool moves = (v > rival[q] || v >= best[q]) && v != INT_MIN;
                        if (__builtin_amdgcn_ballot_w64(moves)) {
                            const unsigned g = gid[i];
                            const bool other = g != best_g[q];
                            const bool nb_ = moves && v >= best[q];                 // later index wins among equals
                            const bool nr = moves && !nb_ && other && v > rival[q];
                            rival[q] = nb_ ? (best_i[q] >= 0 && other ? best[q] : rival[q]) : (nr ? v : rival[q]);
                            best_i[q] = nb_ ? row : best_i[q];
                            best_g[q] = nb_ ? g : best_g[q];
                            best[q] = nb_ ? v : best[q];
                        }
                    }
                }
            }
        }
    }
    // fold the two lane halves' row sets (lanes l and l ^ 32 hold the same a column)
#pragma unroll
    for (int q = 0; q < kGTiles; ++q) {
        const GroupedState mine{best[q], best_i[q], best_g[q], rival[q]};
        const GroupedState theirs{__shfl_xor(best[q], 32), __shfl_xor(best_i[q], 32), (unsigned)__shfl_xor((int)best_g[q], 32),
                                  __shfl_xor(rival[q], 32)};
        const GroupedState st = grouped_merge(mine, theirs);
        const long arow = (a_tile0 + q) * kQTileRows + r;
        if (h == 0 && a_tile0 + q < a_tiles_total && arow < na) {
            if (final) {
                match[arow] = q8_decide(st.best, st.index, st.rival, ratio);
                if (best_out) best_out[arow] = st.best;
                if (rival_out) rival_out[arow] = st.rival;
            } else {
                part[(long)blockIdx.y * na + arow] = make_int4(st.best, st.index, (int)st.group, st.rival);
            }
        }
    }
}

// folds the splits' states of one a row (in ascending split order, which by the merge's definition does not matter) and
// applies the acceptance rule
__global__ __launch_bounds__(256) void match_q8_grouped_merge(const int4 *__restrict__ part, long na, int splits, float ratio,
                                                               int *__restrict__ match, int *__restrict__ best_out,
                                                               int *__restrict__ rival_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    GroupedState st{INT_MIN, -1, 0u, INT_MIN};
    for (int s = 0; s < splits; ++s) {
        const int4 p = part[(long)s * na + i];
        st = grouped_merge(st, GroupedState{p.x, p.y, (unsigned)p.z, p.w});
    }
    match[i] = q8_decide(st.best, st.index, st.rival, ratio);
    if (best_out) best_out[i] = st.best;
    if (rival_out) rival_out[i] = st.rival;
}

// The vote table is zeroed by a kernel of this file, not by a memset: captured in a hipGraph, a memset node of 16 bytes or
// more was seen to replay with a stale 16-byte fill pattern (ROCm 7.2; the table came back holding host addresses plus the
// counts), while the runtime's own stream path and nodes below 16 bytes were right.
__global__ __launch_bounds__(256) void vote_groups_zero(unsigned *__restrict__ votes, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) votes[i] = 0u;
}

// votes [n_groups_a][n_groups_b], zeroed by vote_groups_zero: one integer atomic add per row whose match and both group ids
// are in range.  group_of_a == nullptr: every row is in group 0.
__global__ __launch_bounds__(256) void vote_groups(const int *__restrict__ match, long na,
                                                    const unsigned *__restrict__ group_of_a, unsigned n_groups_a,
                                                    const unsigned *__restrict__ group_of_b, long nb, unsigned n_groups_b,
                                                    unsigned *__restrict__ votes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    const int j = match[i];
    if (j < 0 || j >= nb) return;
    const unsigned ga = group_of_a ? group_of_a[i] : 0u;
    const unsigned gb = group_of_b[j];
    if (ga >= n_groups_a || gb >= n_groups_b) return;
    atomicAdd(votes + (size_t)ga * n_groups_b + gb, 1u);
}

// The grid and the scratch of a call (lf_mkd_match_q8_grouped_plan is this function; launch_match_q8_grouped calls it too):
// match_q8_plan's rule at this kernel's block size.
//   a blocks: kGBlockRows rows each.
//   splits:   1 when all of b is one LDS stage (nb <= 128); otherwise about two workgroups per CU in flight, at least 2 and at
//             most one per b tile (and kGMaxSplits) -- a condition on nb alone, so that for a given b the scratch never falls
//             back to 0 as a grows.  No split is empty.
//   scratch:  16 bytes per (split, a row), stated as  16 * kGBlockRows * min(A + max(W, A), A * b tiles),  W = 2 * CUs,
//             A = a blocks: an upper bound of splits * na (A * ceil(W / A) < W + A and 2 A <= A + max(W, A)) that is
//             non-decreasing in na, and 0 exactly when splits == 1.
Q8GroupedPlan match_q8_grouped_plan(long na, long nb, int num_cus) {
    Q8GroupedPlan p{0, 1, 0, 0};
    if (na <= 0) return p;
    const long a_blocks = (na + kGBlockRows - 1) / kGBlockRows;
    const long b_tiles = (nb + kQTileRows - 1) / kQTileRows;
    const long w = 2L * (num_cus > 0 ? num_cus : 256);
    long splits = 1, per = b_tiles;
    if (b_tiles > kGStage) {
        long want = (w + a_blocks - 1) / a_blocks;
        want = want < 2 ? 2 : want;
        want = want > kGMaxSplits ? kGMaxSplits : want;
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
        p.scratch_bytes = 16ull * kGBlockRows * (unsigned long long)(cap < all ? cap : all);
    }
    return p;
}

unsigned match_q8_grouped_block_rows() { return kGBlockRows; }

void launch_match_q8_grouped(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *group_of_b,
                             const unsigned *excl_lo, const unsigned *excl_hi, float ratio, const Q8GroupedPlan &plan,
                             void *scratch, int *match, int *best, int *rival, hipStream_t stream) {
    if (na <= 0) return;
    int4 *part = static_cast<int4 *>(scratch);
    const int splits = (int)plan.splits;
    hipLaunchKernelGGL(match_q8_grouped_scan, dim3(plan.a_blocks, plan.splits), dim3(kGThreads), 0, stream, a, na, b, nb,
                       plan.tiles_per_split, group_of_b, excl_lo, excl_hi, part, splits == 1 ? 1 : 0, ratio, match, best,
                       rival);
    if (splits > 1)
        hipLaunchKernelGGL(match_q8_grouped_merge, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, stream,
                           (const int4 *)part, na, splits, ratio, match, best, rival);
}

void launch_vote_groups(const int *match, long na, const unsigned *group_of_a, unsigned n_groups_a,
                        const unsigned *group_of_b, long nb, unsigned n_groups_b, unsigned *votes, hipStream_t stream) {
    const long entries = (long)n_groups_a * n_groups_b;
    hipLaunchKernelGGL(vote_groups_zero, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, votes, entries);
    if (na <= 0) return;
    hipLaunchKernelGGL(vote_groups, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, stream, match, na, group_of_a,
                       n_groups_a, group_of_b, nb, n_groups_b, votes);
}

}  // namespace lfmkd
