// gfx950 link tables (include/lf_mkd.h, lf_mkd_link_table_device): the CSR table of the links an edge list's
// match array holds -- per kept edge the list of its correspondences in ascending row order --, the per-edge link counts and
// the match array with everything but the kept edges' links set to -1, made on the device in a fixed number of launches.
//
//   lt_zero      edge_links[e] = 0 (scratch);
//   lt_count     tracks_link's slot map (one workgroup per slot of kSlot entries of ONE edge, so slot order is edge order, then
//                row order): the slot's links (ballot + popcount per wave), its edge, and the edge's total by one integer add;
//   lt_up        the scan over the slots, upwards: per kFan values their sum.  A slot's value is (its links if its edge is
//                selected, 1 if it is the first slot of a selected edge); level 0 is never stored, it is read from lt_count's
//                arrays;
//   lt_down      the scan downwards: per kFan values their exclusive prefix plus the parent's; the top level's one workgroup
//                also leaves the totals and d_counts.  Level 0 leaves per slot W (the links in front) and the selected edges
//                in front;
//   lt_cut       per edge: d_edge_links, and -- by the one selected edge that is the first not kept -- the kept edges and O;
//   lt_scatter   the slot map again: position = the slot's W + the rank within the slot (the lanes in front within the wave,
//                the waves' counts through four words of LDS); d_link_a / d_link_b / d_link_edge and d_match_kept.  Every
//                thread reads its own entry before it writes it: that is what makes d_match_kept == d_match safe;
//   lt_finalise  d_link_offsets[e] = min(W_e, O).
//
// DETERMINISM.  No atomic decides a position: the only atomic is lt_count's integer add into an edge's total, and a sum does
// not depend on its order.  Every scan is an exact integer prefix sum in a fixed order, every rank a count of links in front in
// row order, and launch boundaries are the only ordering between workgroups -- nobody waits, nothing assumes residency.
//
// WHATEVER THE ARRAYS HOLD.  An entry is read or written at lo + r with r < len, (lo, len) from pair_rows against the capacity;
// a link is written at p < min(O, link_capacity) only, and O is only ever stored as a W that the storing thread has compared
// with link_capacity, so d_counts[1] <= link_capacity.  start(e) < slots for every e < n_edges by the formula of the grid.
// For layouts that do not decrease start() increases strictly, every edge owns the slots [start(e), start(e + 1)), W does not
// decrease over the edges and exactly one selected edge is the first not kept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lf_mkd.h"
#include "mkd_block_scan.h"
#include "mkd_device.h"
#include "mkd_match_small.h"        // pair_rows, image_rows, last_pair_at_or_before

#ifndef LF_MKD_LT_SCAN_FANOUT
#define LF_MKD_LT_SCAN_FANOUT 256   // values one workgroup of the slot scan sums: one a thread
#endif

namespace lfmkd {
namespace {

constexpr int kSlot = 256;                                    // entries of one slot = threads of lt_count / lt_scatter:
constexpr int kWaves = kSlot / 64;                            // tracks_link's map, so the two calls split an edge alike
constexpr int kFan = LF_MKD_LT_SCAN_FANOUT;                   // the fan-out of the scan over the slots
constexpr int kEdgeThreads = 256;                             // lt_zero, lt_cut, lt_finalise: one edge a thread
constexpr unsigned kNoEdge = 0xFFFFFFFFu;                     // a slot in front of the first edge
constexpr unsigned kFirst = 0x80000000u;                      // slot_edge: the edge's first slot (n_edges < 2^31: the grid)
static_assert(kFan >= 64 && kFan <= 1024 && (kFan & (kFan - 1)) == 0, "one value a thread, a power of two");

// what a slot is: its edge, the first entry and the number of entries of the edge, the slot's first row within the edge
struct Slot {
    unsigned e;
    long lo, len, r0;
    bool none;                                                // in front of the first edge
};

__device__ __forceinline__ uint64_t slot_start(const uint64_t *__restrict__ edge_off, uint64_t capacity, unsigned p) {
    return (edge_off[p] < capacity ? edge_off[p] : capacity) / kSlot + p;
}

__device__ __forceinline__ Slot slot_of(const uint64_t *__restrict__ edge_off, uint64_t capacity, unsigned n_edges, uint64_t slot) {
    Slot s;
    auto start = [&](unsigned p) { return slot_start(edge_off, capacity, p); };
    s.e = last_pair_at_or_before(n_edges, slot, start);
    pair_rows(edge_off[s.e], edge_off[s.e + 1], capacity, s.lo, s.len);
    const long block = (long)slot - (s.lo / kSlot + (long)s.e);
    s.none = block < 0;
    s.r0 = block * kSlot;
    return s;
}

// the value of slot i in the scan: (links, edges)
__device__ __forceinline__ void leaf_value(const unsigned *__restrict__ slot_cnt, const unsigned *__restrict__ slot_edge,
                                           const unsigned *__restrict__ edge_links, unsigned min_links, long i, uint64_t &links,
                                           uint64_t &edges) {
    links = 0;
    edges = 0;
    const unsigned raw = slot_edge[i];
    if (raw == kNoEdge) return;
    if (edge_links[raw & ~kFirst] < min_links) return;
    links = slot_cnt[i];
    edges = raw >> 31;
}

}  // namespace

// n_edges == 0: no edge; the counts and the one offset are 0
__global__ __launch_bounds__(64) void lt_empty(uint64_t *__restrict__ offsets, unsigned *__restrict__ counts) {
    if (threadIdx.x < 4) counts[threadIdx.x] = 0u;
    if (threadIdx.x == 0) offsets[0] = 0ull;
}

__global__ __launch_bounds__(kEdgeThreads) void lt_zero(unsigned *__restrict__ edge_links, long n_edges) {
    const long e = (long)blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e < n_edges) edge_links[e] = 0u;
}

// Entry lo + r of edge e is a link iff r < min(nA, len) and 0 <= match[lo + r] < nB (tracks_link's rule, with its helpers).
__global__ __launch_bounds__(kSlot) void lt_count(const uint64_t *__restrict__ image_off, unsigned n_images, uint64_t total,
                                                  const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                  const uint64_t *__restrict__ edge_off, uint64_t capacity, unsigned n_edges,
                                                  const int *__restrict__ match, unsigned *__restrict__ slot_cnt,
                                                  unsigned *__restrict__ slot_edge, unsigned *__restrict__ edge_links) {
    __shared__ unsigned s_wave[kWaves];
    const Slot s = slot_of(edge_off, capacity, n_edges, blockIdx.x);
    if (s.none) {                                                // (the same for the whole workgroup, as every return here)
        if (threadIdx.x == 0) {
            slot_cnt[blockIdx.x] = 0u;
            slot_edge[blockIdx.x] = kNoEdge;
        }
        return;
    }
    const unsigned tag = s.e | (s.r0 == 0 ? kFirst : 0u);
    long first_a, na, first_b, nb;
    image_rows(image_off, n_images, total, edge_a[s.e], first_a, na);
    na = na < s.len ? na : s.len;
    if (s.r0 >= na) {                                            // the edge's idle slot(s)
        if (threadIdx.x == 0) {
            slot_cnt[blockIdx.x] = 0u;
            slot_edge[blockIdx.x] = tag;
        }
        return;
    }
    image_rows(image_off, n_images, total, edge_b[s.e], first_b, nb);
    const long r = s.r0 + threadIdx.x;
    bool link = false;
    if (r < na) {
        const int j = match[s.lo + r];
        link = j >= 0 && j < nb;
    }
    const unsigned long long vote = __ballot(link);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = (unsigned)__popcll(vote);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += s_wave[w];
        slot_cnt[blockIdx.x] = sum;
        slot_edge[blockIdx.x] = tag;
        if (sum) atomicAdd(edge_links + s.e, sum);               // a sum: its order does not matter
    }
}

// out[b] = the sum of the kFan values [b kFan, (b + 1) kFan) of the level below.  kLeaf: that level is the slots.
template <bool kLeaf>
__global__ __launch_bounds__(kFan) void lt_up(const unsigned *__restrict__ slot_cnt, const unsigned *__restrict__ slot_edge,
                                              const unsigned *__restrict__ edge_links, unsigned min_links,
                                              const uint64_t *__restrict__ in_links, const unsigned *__restrict__ in_edges,
                                              long n_in, uint64_t *__restrict__ out_links, unsigned *__restrict__ out_edges) {
    __shared__ uint64_t s_scan[2 * kFan];
    const long i = (long)blockIdx.x * kFan + threadIdx.x;
    uint64_t links = 0, edges = 0;
    if (i < n_in) {
        if (kLeaf) {
            leaf_value(slot_cnt, slot_edge, edge_links, min_links, i, links, edges);
        } else {
            links = in_links[i];
            edges = in_edges[i];
        }
    }
    uint64_t total_links, total_edges;
    block_scan<uint64_t, kFan>(links, s_scan, total_links);
    block_scan<uint64_t, kFan>(edges, s_scan, total_edges);
    if (threadIdx.x == 0) {
        out_links[blockIdx.x] = total_links;
        out_edges[blockIdx.x] = (unsigned)total_edges;           // (at most one a slot, slots < 2^31)
    }
}

// The values [b kFan, (b + 1) kFan) of a level become their exclusive prefix plus parent[b] (null: the top level, one
// workgroup, which also stores the totals, counts[2], counts[3], and counts[0], counts[1] as they are if no edge is cut -- 0
// otherwise, until lt_cut's one writer stores them).  kLeaf: the level is the slots, the result goes to slot_base / slot_idx.
template <bool kLeaf>
__global__ __launch_bounds__(kFan) void lt_down(const unsigned *__restrict__ slot_cnt, const unsigned *__restrict__ slot_edge,
                                                const unsigned *__restrict__ edge_links, unsigned min_links,
                                                uint64_t *__restrict__ io_links, unsigned *__restrict__ io_edges, long n_in,
                                                const uint64_t *__restrict__ parent_links, const unsigned *__restrict__ parent_edges,
                                                uint64_t link_capacity, uint64_t *__restrict__ totals, unsigned *__restrict__ counts) {
    __shared__ uint64_t s_scan[2 * kFan];
    const long i = (long)blockIdx.x * kFan + threadIdx.x;
    uint64_t links = 0, edges = 0;
    if (i < n_in) {
        if (kLeaf) {
            leaf_value(slot_cnt, slot_edge, edge_links, min_links, i, links, edges);
        } else {
            links = io_links[i];
            edges = io_edges[i];
        }
    }
    uint64_t total_links, total_edges;
    links = block_scan<uint64_t, kFan>(links, s_scan, total_links);
    edges = block_scan<uint64_t, kFan>(edges, s_scan, total_edges);
    if (parent_links) {
        links += parent_links[blockIdx.x];
        edges += parent_edges[blockIdx.x];
    } else if (threadIdx.x == 0) {
        const bool all = total_links <= link_capacity;
        totals[0] = total_links;
        totals[1] = total_edges;
        counts[0] = all ? (unsigned)total_edges : 0u;
        counts[1] = all ? (unsigned)total_links : 0u;            // (<= link_capacity <= 2^31 - 1)
        counts[2] = (unsigned)total_edges;
        counts[3] = total_links < 0xFFFFFFFFull ? (unsigned)total_links : 0xFFFFFFFFu;
    }
    if (i < n_in) {
        io_links[i] = links;
        io_edges[i] = (unsigned)edges;
    }
}

__global__ __launch_bounds__(kEdgeThreads) void lt_cut(const uint64_t *__restrict__ edge_off, uint64_t capacity, long n_edges,
                                                       const unsigned *__restrict__ links, unsigned min_links,
                                                       const uint64_t *__restrict__ slot_base, const unsigned *__restrict__ slot_idx,
                                                       uint64_t link_capacity, unsigned *__restrict__ edge_links_out,
                                                       unsigned *__restrict__ counts) {
    const long e = (long)blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e >= n_edges) return;
    const unsigned l = links[e];
    if (edge_links_out) edge_links_out[e] = l;
    if (l < min_links) return;
    const uint64_t at = slot_start(edge_off, capacity, (unsigned)e);   // < slots
    const uint64_t w = slot_base[at];
    if (w + l > link_capacity && w <= link_capacity) {          // the selected edges in front are kept, this one is not
        counts[0] = slot_idx[at];
        counts[1] = (unsigned)w;
    }
}

__global__ __launch_bounds__(kSlot) void lt_scatter(const uint64_t *__restrict__ image_off, unsigned n_images, uint64_t total,
                                                    const unsigned *__restrict__ edge_a, const unsigned *__restrict__ edge_b,
                                                    const uint64_t *__restrict__ edge_off, uint64_t capacity, unsigned n_edges,
                                                    const int *match, unsigned min_links, bool local,
                                                    const unsigned *__restrict__ edge_links, const uint64_t *__restrict__ slot_base,
                                                    uint64_t link_capacity, const unsigned *__restrict__ counts,
                                                    int *__restrict__ link_a, int *__restrict__ link_b,
                                                    unsigned *__restrict__ link_edge, int *match_kept) {
    __shared__ unsigned s_wave[kWaves];
    const Slot s = slot_of(edge_off, capacity, n_edges, blockIdx.x);
    if (s.none) return;                                          // (the same for the whole workgroup, as every return here)
    long first_a, na, first_b, nb;
    image_rows(image_off, n_images, total, edge_a[s.e], first_a, na);
    na = na < s.len ? na : s.len;
    if (s.r0 >= na) return;
    image_rows(image_off, n_images, total, edge_b[s.e], first_b, nb);
    const unsigned l = edge_links[s.e];
    const uint64_t w_edge = slot_base[slot_start(edge_off, capacity, s.e)];
    const bool kept = l >= min_links && w_edge + l <= link_capacity;
    const long r = s.r0 + threadIdx.x;
    int j = -1;
    bool link = false;
    if (r < na) {
        j = match[s.lo + r];                                     // read before match_kept, which may be match, is written
        link = kept && j >= 0 && j < nb;
    }
    const unsigned long long vote = __ballot(link);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (unsigned)__popcll(vote);
    __syncthreads();
    if (r >= na) return;
    if (match_kept) match_kept[s.lo + r] = link ? j : -1;        // lo + r < lo + len <= capacity
    if (!link) return;
    uint64_t p = slot_base[blockIdx.x] + (uint64_t)__popcll(vote & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) p += s_wave[w];
    const uint64_t end = (uint64_t)counts[1] < link_capacity ? (uint64_t)counts[1] : link_capacity;
    if (p >= end) return;                                        // (cannot happen for layouts that do not decrease)
    link_a[p] = (int)(local ? r : first_a + r);                  // both below total <= 2^31 - 1
    link_b[p] = (int)(local ? (long)j : first_b + j);
    if (link_edge) link_edge[p] = s.e;
}

// e <= n_edges: d_link_offsets[e] = min(W_e, O); W_{n_edges}: the total
__global__ __launch_bounds__(kEdgeThreads) void lt_finalise(const uint64_t *__restrict__ edge_off, uint64_t capacity, long n_edges,
                                                            const uint64_t *__restrict__ slot_base, const uint64_t *__restrict__ totals,
                                                            const unsigned *__restrict__ counts, uint64_t *__restrict__ offsets) {
    const long e = (long)blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e > n_edges) return;
    const uint64_t w = e < n_edges ? slot_base[slot_start(edge_off, capacity, (unsigned)e)] : totals[0];
    const uint64_t o = counts[1];
    offsets[e] = w < o ? w : o;
}

LinkTablePlan link_table_plan(uint64_t capacity, unsigned n_edges) {
    LinkTablePlan p{};
    p.slot_entries = kSlot;
    p.scan_fanout = kFan;
    p.slots = capacity / kSlot + n_edges;
    if (n_edges == 0) return p;
    p.scan_levels = 1;
    for (uint64_t reach = kFan; reach < p.slots; reach *= kFan) ++p.scan_levels;   // the smallest L with kFan^L >= slots
    // slot_base [slots] u64 | per level k = 1 .. L - 1: links [n_k] u64 | totals [2] u64 | slot_cnt, slot_edge, slot_idx [slots]
    // | per level: edges [n_k] | edge_links [n_edges]
    uint64_t at = p.slots * 8, n = p.slots;
    for (unsigned k = 1; k < p.scan_levels; ++k) {
        n = (n + kFan - 1) / kFan;
        p.level_n[k] = n;
        p.off_level_links[k] = at;
        at += n * 8;
    }
    p.off_totals = at;
    at += 16;
    p.off_slot_cnt = at;
    at += p.slots * 4;
    p.off_slot_edge = at;
    at += p.slots * 4;
    p.off_slot_idx = at;
    at += p.slots * 4;
    for (unsigned k = 1; k < p.scan_levels; ++k) {
        p.off_level_edges[k] = at;
        at += p.level_n[k] * 4;
    }
    p.off_edge_links = at;
    at += (uint64_t)n_edges * 4;
    p.scratch_bytes = at;
    return p;
}

void launch_link_table(const LinkTablePlan &p, unsigned char *scratch, const uint64_t *image_off, unsigned n_images, uint64_t total,
                       const unsigned *edge_a, const unsigned *edge_b, const uint64_t *edge_off, uint64_t capacity, unsigned n_edges,
                       const int *match, unsigned min_links, bool local, uint64_t link_capacity, uint64_t *offsets, int *link_a,
                       int *link_b, unsigned *link_edge, unsigned *edge_links_out, int *match_kept, unsigned *counts,
                       hipStream_t stream) {
    if (n_edges == 0) {
        hipLaunchKernelGGL(lt_empty, dim3(1), dim3(64), 0, stream, offsets, counts);
        return;
    }
    const auto edge_blocks = [](uint64_t items) { return dim3((unsigned)((items + kEdgeThreads - 1) / kEdgeThreads)); };
    const unsigned slots = (unsigned)p.slots;
    const unsigned L = p.scan_levels;
    uint64_t *slot_base = reinterpret_cast<uint64_t *>(scratch);
    uint64_t *totals = reinterpret_cast<uint64_t *>(scratch + p.off_totals);
    unsigned *slot_cnt = reinterpret_cast<unsigned *>(scratch + p.off_slot_cnt);
    unsigned *slot_edge = reinterpret_cast<unsigned *>(scratch + p.off_slot_edge);
    unsigned *slot_idx = reinterpret_cast<unsigned *>(scratch + p.off_slot_idx);
    unsigned *links = reinterpret_cast<unsigned *>(scratch + p.off_edge_links);
    const auto level_links = [&](unsigned k) { return k ? reinterpret_cast<uint64_t *>(scratch + p.off_level_links[k]) : slot_base; };
    const auto level_edges = [&](unsigned k) { return k ? reinterpret_cast<unsigned *>(scratch + p.off_level_edges[k]) : slot_idx; };
    const auto level_n = [&](unsigned k) { return (long)(k ? p.level_n[k] : p.slots); };
    const auto fan_blocks = [](long items) { return dim3((unsigned)((items + kFan - 1) / kFan)); };

    hipLaunchKernelGGL(lt_zero, edge_blocks(n_edges), dim3(kEdgeThreads), 0, stream, links, (long)n_edges);
    hipLaunchKernelGGL(lt_count, dim3(slots), dim3(kSlot), 0, stream, image_off, n_images, total, edge_a, edge_b, edge_off, capacity,
                       n_edges, match, slot_cnt, slot_edge, links);
    for (unsigned k = 1; k < L; ++k) {                           // level k from level k - 1
        if (k == 1)
            hipLaunchKernelGGL(lt_up<true>, fan_blocks(level_n(0)), dim3(kFan), 0, stream, slot_cnt, slot_edge, links, min_links,
                               (const uint64_t *)nullptr, (const unsigned *)nullptr, level_n(0), level_links(1), level_edges(1));
        else
            hipLaunchKernelGGL(lt_up<false>, fan_blocks(level_n(k - 1)), dim3(kFan), 0, stream, slot_cnt, slot_edge, links, min_links,
                               level_links(k - 1), level_edges(k - 1), level_n(k - 1), level_links(k), level_edges(k));
    }
    for (unsigned k = L; k-- > 0;) {                             // level k in place, under level k + 1 (the top: under nothing)
        const uint64_t *parent_links = k + 1 < L ? level_links(k + 1) : nullptr;
        const unsigned *parent_edges = k + 1 < L ? level_edges(k + 1) : nullptr;
        if (k == 0)
            hipLaunchKernelGGL(lt_down<true>, fan_blocks(level_n(0)), dim3(kFan), 0, stream, slot_cnt, slot_edge, links, min_links,
                               slot_base, slot_idx, level_n(0), parent_links, parent_edges, link_capacity, totals, counts);
        else
            hipLaunchKernelGGL(lt_down<false>, fan_blocks(level_n(k)), dim3(kFan), 0, stream, slot_cnt, slot_edge, links, min_links,
                               level_links(k), level_edges(k), level_n(k), parent_links, parent_edges, link_capacity, totals, counts);
    }
    hipLaunchKernelGGL(lt_cut, edge_blocks(n_edges), dim3(kEdgeThreads), 0, stream, edge_off, capacity, (long)n_edges, links,
                       min_links, slot_base, slot_idx, link_capacity, edge_links_out, counts);
    if (link_capacity || match_kept)
        hipLaunchKernelGGL(lt_scatter, dim3(slots), dim3(kSlot), 0, stream, image_off, n_images, total, edge_a, edge_b, edge_off,
                           capacity, n_edges, match, min_links, local, links, slot_base, link_capacity, counts, link_a, link_b,
                           link_edge, match_kept);
    hipLaunchKernelGGL(lt_finalise, edge_blocks((uint64_t)n_edges + 1), dim3(kEdgeThreads), 0, stream, edge_off, capacity,
                       (long)n_edges, slot_base, totals, counts, offsets);
}

}  // namespace lfmkd
