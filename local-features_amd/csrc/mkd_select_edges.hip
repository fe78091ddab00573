// gfx950 candidate edges (include/lf_mkd.h, lf_mkd_select_edges_device): per row of the [n_a][n_b] vote table
// the k best columns -- larger votes first, among equal votes the LOWER column first --, and the edge list those picks make,
// compacted on the device in a fixed number of launches.
//
//   se_select    the table, read once.  Every candidate is ONE 64-bit key,
//                    key = votes << 32 | (0xFFFFFFFF - column)        (column < 2^31, so a key is never 0; 0 is "none")
//                "larger key first" IS the contract's order, a column occurs once per row, so keys are unique, and every merge
//                below is a max-merge of keys: its result cannot depend on the order in which lists arrive.  A lane keeps the K
//                largest keys it has met in a descending register list (static indices only) behind knn_q8_scan's gate: the
//                wave asks ballot(key > list[K - 1]) and only then runs the K-step insertion, once per round for the largest
//                of the 8 keys a lane has loaded, and on rows of three passes or more under a wave-wide floor taken after
//                the first pass (measured beside one gated insertion per key and beside no floor: DESIGN.md 6o).  Rows are read with 16-byte loads
//                between a scalar head and tail that the row's own address decides.  Two forms, chosen by the plan:
//                  kWave   one WAVE per row, four rows a workgroup (rows of at most kWaveRowMax columns);
//                  kBlock  one workgroup per SEGMENT of a row (a whole row, or 1 / splits of it when there are too few rows
//                          to fill the device); the waves' lists meet in LDS.
//                The lanes' lists are merged by k rounds of "wave maximum of the heads, the owner pops".
//   se_merge     splits > 1 only: one wave per row max-merges the segments' k keys, in the same way.
//   se_flag      one thread per pick slot (row, rank): is it an edge?  Under UNIQUE that is k reads of the rank table.  The
//                workgroup's 256 flags are ranked (ballot + popcount, four words of LDS) and counted.
//   se_scan      ONE workgroup: the exclusive prefix of the workgroups' edge counts, the three totals, d_counts.
//   se_scatter   position = the workgroup's prefix + the rank within it; the padding behind the edges.
//
// DETERMINISM.  No atomic at all.  Every selection is a maximum of unique keys, every position an exact integer prefix in a
// fixed order, and launch boundaries are the only ordering between workgroups -- nobody waits, nothing assumes residency.
//
// BOUNDS.  A row's segment [c0, c1) is read at votes + i n_b + c with c0 <= c < c1 <= n_b only: the 16-byte loads cover the
// part of it between the first and the last 16-byte boundary inside it.  Ranks are written at i k + c, c < k, i < n_a; edges
// at p < edge_capacity.  Under UNIQUE n_a == n_b, so a picked column is a row of the rank table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lf_mkd.h"
#include "mkd_block_scan.h"
#include "mkd_device.h"

namespace lfmkd {
namespace {

constexpr int kThreads = 256;                                 // every kernel here but se_scan
constexpr int kWaves = kThreads / 64;
constexpr unsigned kWaveRowMax = 2048;                        // the longest row one wave takes: 8 16-byte loads a lane
constexpr unsigned kMinSegment = 4096;                        // the shortest segment a row is split into: 4 loads a thread
constexpr uint64_t kTargetGroups = 1024;                      // rows are split while there are fewer workgroups than this
constexpr int kScanThreads = 1024;                            // se_scan: workgroup counts per pass
constexpr unsigned kNoPick = 0xFFFFFFFFu;                     // se_flag's local position of a slot that is no edge
constexpr unsigned kPad = 0xFFFFFFFFu;                        // the padding of d_edge_a / d_edge_b: an empty image

typedef unsigned long long key_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // a 16-byte load

__device__ __forceinline__ key_t make_key(unsigned votes, unsigned column) { return ((key_t)votes << 32) | (key_t)(0xFFFFFFFFu - column); }
__device__ __forceinline__ int key_column(key_t key) { return key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1; }
__device__ __forceinline__ unsigned key_votes(key_t key) { return (unsigned)(key >> 32); }

// key into the descending list: list[j] = max(list[j], min(list[j - 1], key)), from the tail up.  A key that is not above
// list[K - 1] -- 0 among them -- changes nothing.
template <int K>
__device__ __forceinline__ void list_insert(key_t (&list)[K], key_t key) {
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        const key_t up = list[j - 1] < key ? list[j - 1] : key;
        list[j] = list[j] > up ? list[j] : up;
    }
    list[0] = list[0] > key ? list[0] : key;
}

template <int K>
__device__ __forceinline__ void list_offer(key_t (&list)[K], key_t key) {
    if (__builtin_amdgcn_ballot_w64(key > list[K - 1])) list_insert<K>(list, key);
}

__device__ __forceinline__ key_t wave_max(key_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, off, 64), hi = __shfl_xor((unsigned)(x >> 32), off, 64);
        const key_t y = ((key_t)hi << 32) | lo;
        x = y > x ? y : x;
    }
    return x;
}

// The wave's next largest key: the maximum of the lanes' heads; its one owner (keys are unique) pops it.  0: none left.
template <int L>
__device__ __forceinline__ key_t wave_pop(key_t (&list)[L]) {
    const key_t m = wave_max(list[0]);
    const bool pop = list[0] == m;
#pragma unroll
    for (int j = 0; j + 1 < L; ++j) list[j] = pop ? list[j + 1] : list[j];
    list[L - 1] = pop ? 0ull : list[L - 1];
    return m;
}

struct RowRule {
    unsigned min_votes, self;                                 // self: the column that is no candidate (kNoPick: none)
};

__device__ __forceinline__ key_t candidate(const RowRule &rule, unsigned votes, unsigned column, bool inside) {
    return inside && votes >= rule.min_votes && column != rule.self ? make_key(votes, column) : 0ull;
}

// The columns [c0, c1) of the row at `row`, by NT threads of which this is thread t: a scalar head up to the first 16-byte
// boundary, 16-byte loads (two in flight), a scalar tail.  Every trip count is the same for all NT threads.
template <int K, int NT>
__device__ __forceinline__ void scan_votes(key_t (&list)[K], const unsigned *__restrict__ row, unsigned c0, unsigned c1,
                                           const RowRule &rule, int t) {
    const unsigned *p = row + c0;
    const unsigned len = c1 - c0;
    unsigned head = (unsigned)((0u - (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2)) & 3u);
    head = head < len ? head : len;
    const unsigned n_vec = (len - head) >> 2, tail0 = head + (n_vec << 2);
    {
        const bool in = (unsigned)t < head;                       // (head <= 3)
        list_offer<K>(list, candidate(rule, in ? p[t] : 0u, c0 + t, in));
    }
    const u32x4 *pv = reinterpret_cast<const u32x4 *>(p + head);
    // The wave's floor: a key below K other keys of the wave's own columns is none of the row's K best, whichever lane
    // meets it.  After the first pass every lane's largest key is known; the K-th largest of those 64 is such a floor (0
    // while fewer than K lanes hold a key), and it closes the gate for lanes whose own lists are still short or weak.
    key_t floor = 0ull;
    const bool floored = n_vec > 4 * NT;                          // (the same for the whole wave; it pays from three passes on)
    for (unsigned v0 = 0; v0 < n_vec; v0 += 2 * NT) {
        const unsigned va = v0 + t, vb = va + NT;
        const bool in_a = va < n_vec, in_b = vb < n_vec;
        u32x4 qa = {0u, 0u, 0u, 0u}, qb = qa;
        if (in_a) qa = __builtin_nontemporal_load(pv + va);
        if (in_b) qb = __builtin_nontemporal_load(pv + vb);
        const unsigned ja = c0 + head + (va << 2), jb = c0 + head + (vb << 2);
        key_t key[8] = {candidate(rule, qa.x, ja, in_a),     candidate(rule, qa.y, ja + 1, in_a),
                        candidate(rule, qa.z, ja + 2, in_a), candidate(rule, qa.w, ja + 3, in_a),
                        candidate(rule, qb.x, jb, in_b),     candidate(rule, qb.y, jb + 1, in_b),
                        candidate(rule, qb.z, jb + 2, in_b), candidate(rule, qb.w, jb + 3, in_b)};
        key_t m = key[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) m = key[q] > m ? key[q] : m;
        // The first pass, and on rows too short for a floor the first K / 8 passes: the lists are not full, nearly every
        // key enters, and eight gated insertions in any order cost less than rounds.
        if (v0 == 0 || (!floored && 4 * v0 < (unsigned)K * NT)) {
#pragma unroll
            for (int q = 0; q < 8; ++q) list_offer<K>(list, key[q]);
            m = 0ull;
        }
        // Rounds: every lane inserts the largest key it still holds, while any lane holds one that enters -- as many
        // insertions as the busiest lane has entering keys, not one per key; none once the scan is under way.  (Eight gated
        // rounds in sequence rather than a loop: a closed gate stays closed, and the list is not carried round a back edge.)
#pragma unroll
        for (int round = 0; round < 8; ++round) {
            const key_t bar = list[K - 1] > floor ? list[K - 1] : floor;
            if (__builtin_amdgcn_ballot_w64(m > bar)) {
                list_insert<K>(list, m);                          // (a key that does not enter changes nothing)
                key_t next = 0ull;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    key[q] = key[q] == m ? 0ull : key[q];         // keys are unique
                    next = key[q] > next ? key[q] : next;
                }
                m = next;
            }
        }
        if (v0 == 0 && floored) {
            key_t top = list[0];
            for (int r = 0; r < K; ++r) {
                floor = wave_max(top);
                top = top == floor ? 0ull : top;
            }
        }
    }
    {
        const bool in = (unsigned)t < len - tail0;                // (at most 3)
        list_offer<K>(list, candidate(rule, in ? p[tail0 + t] : 0u, c0 + tail0 + t, in));
    }
}

// rank c of row i, to the rank table -- or, for one segment of a split row, to the segment's keys
__device__ __forceinline__ void store_pick(key_t key, long at, int *__restrict__ rank, unsigned *__restrict__ rank_votes,
                                           key_t *__restrict__ part) {
    if (part) {
        part[at] = key;
    } else {
        rank[at] = key_column(key);
        rank_votes[at] = key_votes(key);
    }
}

}  // namespace

// kWave: workgroup b's wave w owns row 4 b + w.  Otherwise: workgroup b owns segment b % splits of row b / splits and writes
// its k keys to part[(row splits + segment) k + c] (splits == 1: the ranks themselves).
template <int K, bool kWave>
__global__ __launch_bounds__(kThreads) void se_select(const unsigned *__restrict__ votes, unsigned n_a, unsigned n_b, unsigned k,
                                                      unsigned min_votes, bool skip_self, unsigned splits, unsigned segment,
                                                      int *__restrict__ rank, unsigned *__restrict__ rank_votes,
                                                      key_t *__restrict__ part) {
    constexpr int L = K * kWaves > 64 ? K * kWaves / 64 : 1;      // keys a lane of wave 0 takes from the waves' lists
    __shared__ key_t s_keys[kWave ? 1 : 64 * L];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    key_t list[K];
#pragma unroll
    for (int j = 0; j < K; ++j) list[j] = 0ull;
    if (kWave) {
        const long i = (long)blockIdx.x * kWaves + wave;
        if (i >= n_a) return;                                     // (the whole wave)
        const RowRule rule = {min_votes, skip_self ? (unsigned)i : kNoPick};
        scan_votes<K, 64>(list, votes + (size_t)i * n_b, 0u, n_b, rule, lane);
        for (unsigned c = 0; c < k; ++c) {
            const key_t m = wave_pop<K>(list);
            if (lane == 0) store_pick(m, i * k + c, rank, rank_votes, nullptr);
        }
    } else {
        const unsigned i = blockIdx.x / splits, s = blockIdx.x - i * splits;
        const unsigned c0 = s * segment;                          // < n_b: the plan's splits = ceil(n_b / segment)
        const unsigned c1 = n_b - c0 > segment ? c0 + segment : n_b;
        const RowRule rule = {min_votes, skip_self ? i : kNoPick};
        scan_votes<K, kThreads>(list, votes + (size_t)i * n_b, c0, c1, rule, (int)threadIdx.x);
        for (int x = threadIdx.x; x < 64 * L; x += kThreads) s_keys[x] = 0ull;
        __syncthreads();
        for (unsigned c = 0; c < k; ++c) {
            const key_t m = wave_pop<K>(list);
            if (lane == 0) s_keys[wave * K + c] = m;
        }
        __syncthreads();
        if (wave != 0) return;
        key_t mine[L];
#pragma unroll
        for (int j = 0; j < L; ++j) mine[j] = 0ull;
#pragma unroll
        for (int j = 0; j < L; ++j) list_insert<L>(mine, s_keys[j * 64 + lane]);
        const long at = ((long)i * splits + s) * k;
        for (unsigned c = 0; c < k; ++c) {
            const key_t m = wave_pop<L>(mine);
            if (lane == 0) store_pick(m, at + c, rank, rank_votes, splits > 1 ? part : nullptr);
        }
    }
}

// splits > 1: one wave per row, the k best of its segments' splits * k keys
template <int K>
__global__ __launch_bounds__(kThreads) void se_merge(const key_t *__restrict__ part, unsigned n_a, unsigned k, unsigned splits,
                                                     int *__restrict__ rank, unsigned *__restrict__ rank_votes) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * kWaves + wave;
    if (i >= n_a) return;                                         // (the whole wave)
    key_t list[K];
#pragma unroll
    for (int j = 0; j < K; ++j) list[j] = 0ull;
    const unsigned n = splits * k;                                // <= 1024 * 32
    const key_t *mine = part + i * n;
    for (unsigned x0 = 0; x0 < n; x0 += 64) {
        const unsigned x = x0 + lane;
        list_offer<K>(list, x < n ? mine[x] : 0ull);
    }
    for (unsigned c = 0; c < k; ++c) {
        const key_t m = wave_pop<K>(list);
        if (lane == 0) store_pick(m, i * k + c, rank, rank_votes, nullptr);
    }
}

// Slot p = i k + c is a PICK iff rank[p] >= 0, and an EDGE iff it is a pick and -- under kUnique -- its column j is above i,
// or below i with i not among row j's picks.  local[p] = the edges in front of p within the workgroup (kNoPick: no edge).
__global__ __launch_bounds__(kThreads) void se_flag(const int *__restrict__ rank, long n_slots, unsigned k, bool unique,
                                                    unsigned *__restrict__ local, unsigned *__restrict__ block_edges,
                                                    unsigned *__restrict__ block_picks, unsigned *__restrict__ block_rows) {
    __shared__ unsigned s_wave[3][kWaves];
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool pick = false, edge = false, first = false;
    if (p < n_slots) {
        const int j = rank[p];
        const long i = p / k;
        pick = j >= 0;
        first = pick && p == i * k;
        edge = pick;
        if (unique && pick) {
            edge = j != i;
            if (j < i) {
                const int *theirs = rank + (long)j * k;           // j < i < n_a
                for (unsigned c = 0; c < k; ++c) edge = edge && theirs[c] != (int)i;
            }
        }
    }
    const unsigned long long edges = __builtin_amdgcn_ballot_w64(edge);
    const unsigned long long picks = __builtin_amdgcn_ballot_w64(pick);
    const unsigned long long rows = __builtin_amdgcn_ballot_w64(first);
    if (lane == 0) {
        s_wave[0][wave] = (unsigned)__popcll(edges);
        s_wave[1][wave] = (unsigned)__popcll(picks);
        s_wave[2][wave] = (unsigned)__popcll(rows);
    }
    __syncthreads();
    unsigned at = (unsigned)__popcll(edges & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) at += s_wave[0][w];
    if (p < n_slots) local[p] = edge ? at : kNoPick;
    if (threadIdx.x == 0) {
        unsigned sum[3] = {0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            sum[0] += s_wave[0][w];
            sum[1] += s_wave[1][w];
            sum[2] += s_wave[2][w];
        }
        block_edges[blockIdx.x] = sum[0];
        block_picks[blockIdx.x] = sum[1];
        block_rows[blockIdx.x] = sum[2];
    }
}

// ONE workgroup: block_base[b] = the edges of the workgroups in front of b, in passes of kScanThreads with a carry; the
// totals (all at most n_a k <= 2^31 - 1) and d_counts.
__global__ __launch_bounds__(kScanThreads) void se_scan(const unsigned *__restrict__ block_edges,
                                                        const unsigned *__restrict__ block_picks,
                                                        const unsigned *__restrict__ block_rows, long n_blocks,
                                                        uint64_t edge_capacity, unsigned *__restrict__ block_base,
                                                        unsigned *__restrict__ counts) {
    __shared__ unsigned s_scan[2 * kScanThreads];
    __shared__ unsigned s_sum[2][kScanThreads / 64];
    const int t = threadIdx.x;
    unsigned carry = 0, picks = 0, rows = 0;
    for (long b0 = 0; b0 < n_blocks; b0 += kScanThreads) {
        const long b = b0 + t;
        const unsigned v = b < n_blocks ? block_edges[b] : 0u;
        if (b < n_blocks) {
            picks += block_picks[b];
            rows += block_rows[b];
        }
        unsigned total;
        const unsigned before = block_scan<unsigned, kScanThreads>(v, s_scan, total);
        if (b < n_blocks) block_base[b] = carry + before;
        carry += total;
    }
    // the two plain totals: a sum over the lanes, then over the waves
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        picks += __shfl_xor(picks, off, 64);
        rows += __shfl_xor(rows, off, 64);
    }
    if ((t & 63) == 0) {
        s_sum[0][t >> 6] = picks;
        s_sum[1][t >> 6] = rows;
    }
    __syncthreads();
    if (t == 0) {
        picks = 0;
        rows = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {
            picks += s_sum[0][w];
            rows += s_sum[1][w];
        }
        counts[0] = (uint64_t)carry < edge_capacity ? carry : (unsigned)edge_capacity;
        counts[1] = carry;
        counts[2] = picks;
        counts[3] = rows;
    }
}

// Thread p: slot p's edge, if it is one and its position is below edge_capacity; and the padding at position p, if p is at
// or beyond the edges (counts[1], from se_scan) and below edge_capacity.  The two sets of positions are disjoint.
__global__ __launch_bounds__(kThreads) void se_scatter(const int *__restrict__ rank, const unsigned *__restrict__ rank_votes,
                                                       const unsigned *__restrict__ local, const unsigned *__restrict__ block_base,
                                                       long n_slots, unsigned k, bool unique, uint64_t edge_capacity,
                                                       const unsigned *__restrict__ counts, unsigned *__restrict__ edge_a,
                                                       unsigned *__restrict__ edge_b, unsigned *__restrict__ edge_votes) {
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p < n_slots) {
        const unsigned at = local[p];
        if (at != kNoPick) {
            const uint64_t e = (uint64_t)block_base[blockIdx.x] + at;
            if (e < edge_capacity) {
                const unsigned i = (unsigned)(p / k), j = (unsigned)rank[p];
                const bool swap = unique && j < i;
                edge_a[e] = swap ? j : i;
                edge_b[e] = swap ? i : j;
                if (edge_votes) edge_votes[e] = rank_votes[p];
            }
        }
    }
    if ((uint64_t)p < edge_capacity && (uint64_t)p >= (uint64_t)counts[1]) {
        edge_a[p] = kPad;
        edge_b[p] = kPad;
        if (edge_votes) edge_votes[p] = 0u;
    }
}

// n_a == 0: no pick; the counts are 0 and every edge is padding
__global__ __launch_bounds__(kThreads) void se_empty(uint64_t edge_capacity, unsigned *__restrict__ edge_a,
                                                     unsigned *__restrict__ edge_b, unsigned *__restrict__ edge_votes,
                                                     unsigned *__restrict__ counts) {
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p < 4) counts[p] = 0u;
    if ((uint64_t)p < edge_capacity) {
        edge_a[p] = kPad;
        edge_b[p] = kPad;
        if (edge_votes) edge_votes[p] = 0u;
    }
}

SelectEdgesPlan select_edges_plan(unsigned n_a, unsigned n_b, unsigned k, uint64_t edge_capacity) {
    SelectEdgesPlan p{};
    p.compiled_k = k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32;
    p.rows_per_workgroup = n_b <= kWaveRowMax ? kWaves : 1;
    p.splits = 1;
    p.segment = n_b;
    if (n_a == 0) {
        p.workgroups = 0;
        p.launches = 1;
        return p;
    }
    if (p.rows_per_workgroup == 1 && n_a < kTargetGroups) {
        // as many segments as fill the device, none shorter than kMinSegment, each a multiple of 4 columns
        uint64_t want = (kTargetGroups + n_a - 1) / n_a;
        const uint64_t most = (n_b + kMinSegment - 1) / kMinSegment;
        want = want < most ? want : most;
        const uint64_t seg = (((uint64_t)n_b + want - 1) / want + 3) & ~3ull;
        p.segment = (unsigned)seg;
        p.splits = (unsigned)((n_b + seg - 1) / seg);
    }
    p.workgroups = p.rows_per_workgroup == 1 ? (uint64_t)n_a * p.splits : ((uint64_t)n_a + kWaves - 1) / kWaves;
    p.launches = p.splits > 1 ? 5 : 4;
    p.slots = (uint64_t)n_a * k;
    p.blocks = (p.slots + kThreads - 1) / kThreads;
    // part [n_a splits k] u64 (splits > 1) | rank, rank_votes, local [slots] | block_edges, _picks, _rows, _base [blocks]
    uint64_t at = p.splits > 1 ? (uint64_t)n_a * p.splits * k * 8 : 0;
    p.off_rank = at;
    at += p.slots * 4;
    p.off_rank_votes = at;
    at += p.slots * 4;
    p.off_local = at;
    at += p.slots * 4;
    p.off_blocks = at;
    at += p.blocks * 16;
    p.scratch_bytes = at;
    (void)edge_capacity;
    return p;
}

namespace {

template <int K>
void launch_select(const SelectEdgesPlan &p, const unsigned *votes, unsigned n_a, unsigned n_b, unsigned k, unsigned min_votes,
                   bool skip_self, int *rank, unsigned *rank_votes, key_t *part, hipStream_t stream) {
    if (p.rows_per_workgroup != 1) {
        hipLaunchKernelGGL((se_select<K, true>), dim3((unsigned)p.workgroups), dim3(kThreads), 0, stream, votes, n_a, n_b, k,
                           min_votes, skip_self, 1u, n_b, rank, rank_votes, (key_t *)nullptr);
        return;
    }
    hipLaunchKernelGGL((se_select<K, false>), dim3((unsigned)p.workgroups), dim3(kThreads), 0, stream, votes, n_a, n_b, k,
                       min_votes, skip_self, p.splits, p.segment, rank, rank_votes, part);
    if (p.splits > 1)
        hipLaunchKernelGGL((se_merge<K>), dim3((n_a + kWaves - 1) / kWaves), dim3(kThreads), 0, stream, (const key_t *)part, n_a, k,
                           p.splits, rank, rank_votes);
}

}  // namespace

void launch_select_edges(const SelectEdgesPlan &p, unsigned char *scratch, const unsigned *votes, unsigned n_a, unsigned n_b,
                         unsigned k, unsigned min_votes, bool skip_self, bool unique, uint64_t edge_capacity, int *rank,
                         unsigned *rank_votes, unsigned *edge_a, unsigned *edge_b, unsigned *edge_votes, unsigned *counts,
                         hipStream_t stream) {
    const auto blocks_of = [](uint64_t items) { return dim3((unsigned)((items + kThreads - 1) / kThreads)); };
    if (n_a == 0) {
        hipLaunchKernelGGL(se_empty, blocks_of(edge_capacity > 4 ? edge_capacity : 4), dim3(kThreads), 0, stream, edge_capacity,
                           edge_a, edge_b, edge_votes, counts);
        return;
    }
    key_t *part = reinterpret_cast<key_t *>(scratch);
    if (!rank) rank = reinterpret_cast<int *>(scratch + p.off_rank);
    if (!rank_votes) rank_votes = reinterpret_cast<unsigned *>(scratch + p.off_rank_votes);
    unsigned *local = reinterpret_cast<unsigned *>(scratch + p.off_local);
    unsigned *block_edges = reinterpret_cast<unsigned *>(scratch + p.off_blocks);
    unsigned *block_picks = block_edges + p.blocks, *block_rows = block_picks + p.blocks, *block_base = block_rows + p.blocks;
    switch (p.compiled_k) {
    case 4: launch_select<4>(p, votes, n_a, n_b, k, min_votes, skip_self, rank, rank_votes, part, stream); break;
    case 8: launch_select<8>(p, votes, n_a, n_b, k, min_votes, skip_self, rank, rank_votes, part, stream); break;
    case 16: launch_select<16>(p, votes, n_a, n_b, k, min_votes, skip_self, rank, rank_votes, part, stream); break;
    default: launch_select<32>(p, votes, n_a, n_b, k, min_votes, skip_self, rank, rank_votes, part, stream); break;
    }
    hipLaunchKernelGGL(se_flag, dim3((unsigned)p.blocks), dim3(kThreads), 0, stream, (const int *)rank, (long)p.slots, k, unique,
                       local, block_edges, block_picks, block_rows);
    hipLaunchKernelGGL(se_scan, dim3(1), dim3(kScanThreads), 0, stream, (const unsigned *)block_edges, (const unsigned *)block_picks,
                       (const unsigned *)block_rows, (long)p.blocks, edge_capacity, block_base, counts);
    const uint64_t reach = p.slots > edge_capacity ? p.slots : edge_capacity;
    hipLaunchKernelGGL(se_scatter, blocks_of(reach), dim3(kThreads), 0, stream, (const int *)rank, (const unsigned *)rank_votes,
                       (const unsigned *)local, (const unsigned *)block_base, (long)p.slots, k, unique, edge_capacity,
                       (const unsigned *)counts, edge_a, edge_b, edge_votes);
}

}  // namespace lfmkd
