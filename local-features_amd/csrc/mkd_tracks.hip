// gfx950 feature tracks (include/lf_mkd.h, lf_mkd_build_tracks_device): the connected components of the links
// an edge list's match array holds between the rows of one pool, one label per pool row, and per track its length and its
// number of conflicting rows.  A lock-free union-find whose forest lives in the output itself:
//
//   tracks_init     track[r] = r (not under LF_MKD_TRACKS_ACCUMULATE: the array is then the forest an earlier call left);
//   tracks_link     one thread per entry of the a side's edge layout; a link joins two trees with one compare-and-swap;
//   tracks_flatten  track[r] = the root of r, in place;
//   tracks_zero, tracks_len, tracks_dup   the statistics, integer atomics only.
//
// THE FOREST.  track[x] is x's parent, and parent <= index always: an entry p at index x with p < 0 || p > x is read as x
// (clamp_parent), which is how an array of anything is a forest under ACCUMULATE.  Every walk therefore descends and ends.
// A link only ever hangs the LARGER of two roots under the smaller one, so a root is the minimum of its tree -- and once all
// links are in, the trees are the components, so a row's label is its component's smallest row whatever the order the links
// were taken in.  That is the whole determinism argument; nothing here depends on the order of the edges, on the dispatch
// order or on the CU count.
//
// NOBODY WAITS.  No workgroup ever waits for another one: no flag, no spin on somebody else's progress, no assumption on which
// workgroups are resident together.  The only loop that repeats on account of other threads is tracks_link's, and it is
// bounded by the descent alone (see there).
//
// dup's cost is quadratic in one image's row count (a row is compared with the labels of the rows of its image in front of
// it): at the 500 .. 8000 rows an image has here that is 0.1 .. 32 M integer compares an image, next to nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lf_mkd.h"   // LF_MKD_TRACKS_DUP_TILE
#include "mkd_device.h"
#include "mkd_match_small.h"        // pair_rows, image_rows, last_pair_at_or_before

namespace lfmkd {
namespace {

constexpr int kRowThreads = 256;                        // rows one workgroup of init / flatten / zero / len serves
constexpr int kLinkEntries = 256;                       // layout entries one workgroup of tracks_link serves, one a thread
constexpr int kDupTile = LF_MKD_TRACKS_DUP_TILE;        // rows one workgroup of tracks_dup serves = labels per LDS tile
static_assert(kDupTile % 4 == 0 && kDupTile <= 1024, "tracks_dup reads its tile four labels at a time, one thread a row");

// EVERY read and write of a parent while the forest changes is an agent-scope atomic (global_load / global_store ... sc1,
// served by L2): a plain load may be served from this CU's L1, which no other CU's store ever refreshes.
__device__ __forceinline__ int load_entry(const int *track, int x) {
    return __hip_atomic_load(track + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_entry(int *track, int x, int v) {
    __hip_atomic_store(track + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int clamp_parent(int p, int x) { return (p < 0 || p > x) ? x : p; }

// The root of x's tree as far as the entries read say, and `raw`, what that root's own entry held (the root itself, or under
// ACCUMULATE anything clamp_parent reads as the root).  Path halving: a row that is no root gets its grandparent, which is
// still an ancestor and still below it; no compare-and-swap can succeed on such a row (it expects a root's entry, and a row
// that has a parent never becomes a root again), so a plain atomic store is enough.
__device__ __forceinline__ int find_root(int *track, int x, int &raw) {
    raw = load_entry(track, x);
    int p = clamp_parent(raw, x);
    while (p != x) {
        const int raw_p = load_entry(track, p);
        const int g = clamp_parent(raw_p, p);
        if (g == p) {                                   // p is the root
            x = p;
            raw = raw_p;
            break;
        }
        store_entry(track, x, g);
        x = g;
        raw = load_entry(track, x);
        p = clamp_parent(raw, x);
    }
    return x;
}

}  // namespace

__global__ __launch_bounds__(kRowThreads) void tracks_init(int *__restrict__ track, long n) {
    const long r = (long)blockIdx.x * kRowThreads + threadIdx.x;
    if (r < n) track[r] = (int)r;
}

// One thread per entry of the a side's edge layout: gather_edge_rows' slot map over the layout against its capacity at
// kLinkEntries entries a slot, floor(capacity / kLinkEntries) + n_edges workgroups.  Entry lo + r of edge e is a link between
// pool rows firstA + r and firstB + j, j = match[lo + r], iff r < min(nA, len) and 0 <= j < nB.
__global__ __launch_bounds__(kLinkEntries) void tracks_link(const uint64_t *__restrict__ image_off, unsigned n_images,
                                                            uint64_t total, const unsigned *__restrict__ edge_a,
                                                            const unsigned *__restrict__ edge_b,
                                                            const uint64_t *__restrict__ edge_off, uint64_t capacity,
                                                            unsigned n_edges, const int *__restrict__ match, int *track) {
    const uint64_t slot = blockIdx.x;
    auto start = [&](unsigned p) { return (edge_off[p] < capacity ? edge_off[p] : capacity) / kLinkEntries + p; };
    const unsigned e = last_pair_at_or_before(n_edges, slot, start);
    long lo, len, first_a, na, first_b, nb;
    pair_rows(edge_off[e], edge_off[e + 1], capacity, lo, len);
    const long block = (long)slot - (lo / kLinkEntries + (long)e);
    if (block < 0) return;                                       // entries in front of the first edge
    image_rows(image_off, n_images, total, edge_a[e], first_a, na);
    na = na < len ? na : len;
    const long r = block * kLinkEntries + threadIdx.x;
    if (r >= na) return;                                         // the edge's idle slot(s), the tail of its last one
    image_rows(image_off, n_images, total, edge_b[e], first_b, nb);
    const int j = match[lo + r];
    if (j < 0 || j >= nb) return;                                // no link
    int u = (int)(first_a + r), v = (int)(first_b + j);          // both below total <= 2^31 - 1
    // Join u's tree and v's.  Every entry ever read for a row is a row of that row's own tree (a parent, or a grandparent an
    // earlier halving stored), and trees only grow, so whatever mixture of old and new entries a walk meets it ends at a row
    // of the right tree; ending at the SAME row on both sides means the two are joined already.  The compare-and-swap
    // succeeds only if hi's entry still is what a root's entry is, i.e. if hi really is the root of its whole tree at that
    // moment; it then hangs under a smaller row of the other tree, so parent < index stays true and a root stays the minimum
    // of its tree.
    // The loop is finite on its own account: a failed compare-and-swap means somebody else lowered track[hi] (or, under
    // ACCUMULATE, that the entry held another out-of-range value than the one read, which is retried at once with what the
    // swap returned), and the walk goes on from the parent THE SWAP ITSELF RETURNED and from lo, both strictly below hi --
    // max(u, v) falls with every round.  It goes on from the swap's answer and not from a fresh read on purpose: were the
    // reads plain loads, a thread could keep seeing "hi is a root" in its CU's stale L1 line after the swap in L2 said
    // otherwise and never finish; the agent-scope loads make the reads fresh, the swap's answer makes the bound independent
    // of them.
    for (;;) {
        int raw_u, raw_v;
        const int ru = find_root(track, u, raw_u), rv = find_root(track, v, raw_v);
        if (ru == rv) return;
        const int hi = ru > rv ? ru : rv, low = ru > rv ? rv : ru;
        int seen = ru > rv ? raw_u : raw_v;
        for (;;) {
            if (__hip_atomic_compare_exchange_strong(track + hi, &seen, low, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                return;
            if (clamp_parent(seen, hi) != hi) break;             // hi has a parent now: seen
        }
        u = seen;
        v = low;
    }
}

// track[r] = the root of r.  No link is taken in this launch, so the roots are fixed, and every value stored -- a root -- is
// an ancestor of the row it is stored at: a walk that meets old and new entries mixed still ends at the row's root.  (No
// path halving here: a grandparent stored at r behind r's own final store would undo it.)
__global__ __launch_bounds__(kRowThreads) void tracks_flatten(int *track, long n) {
    const long r = (long)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= n) return;
    int x = (int)r;
    for (;;) {
        const int p = clamp_parent(load_entry(track, x), x);
        if (p == x) break;
        x = p;
    }
    store_entry(track, (int)r, x);
}

__global__ __launch_bounds__(kRowThreads) void tracks_zero(unsigned *__restrict__ len, unsigned *__restrict__ dup, long n) {
    const long r = (long)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= n) return;
    if (len) len[r] = 0u;
    if (dup) dup[r] = 0u;
}

// counter[t] += 1 for every lane that is `on` (called by whole waves).  The lanes that share the label of the wave's first
// counting lane add once, together: one long track is the common case of a matched collection, and its rows would otherwise
// queue on one address one by one.
__device__ __forceinline__ void count_label(unsigned *__restrict__ counter, int t, bool on) {
    const unsigned long long live = __ballot(on);
    if (live == 0) return;                                       // (wave-uniform)
    const int t0 = __builtin_amdgcn_readlane(t, __ffsll((long long)live) - 1);
    const bool same = on && t == t0;
    const unsigned long long mask = __ballot(same);
    if (same) {
        if ((mask & ((1ull << (threadIdx.x & 63)) - 1)) == 0) atomicAdd(counter + t, (unsigned)__popcll(mask));
    } else if (on) {
        atomicAdd(counter + t, 1u);
    }
}

// len[track[r]] += 1 per row
__global__ __launch_bounds__(kRowThreads) void tracks_len(const int *__restrict__ track, long n, unsigned *__restrict__ len) {
    const long r = (long)blockIdx.x * kRowThreads + threadIdx.x;
    const bool on = r < n;
    count_label(len, on ? track[r] : -1, on);
}

// dup[t] = the sum over images m of max(c(m, t) - 1, 0) = the number of (image, row of it) whose label occurs at a LOWER row
// of the same image.  The grid is the slot map of the image offsets against the total at kDupTile rows a slot,
// floor(total / kDupTile) + n_images workgroups; a workgroup streams the labels of its image's rows in front of its own
// rows, and then its own, through LDS in tiles of kDupTile, every thread comparing its own row's label with each (four labels
// an LDS read, the same address in every lane).  A wave none of whose rows is still looking skips the compares of a tile,
// not its loads and barriers.
// len (nullable): the finished lengths; a row whose track has length 1 has nothing to find.  The skip is taken only when the
// caller asked for d_track_len -- without it there is nowhere to keep the lengths, and every row scans.
__global__ __launch_bounds__(kDupTile) void tracks_dup(const uint64_t *__restrict__ image_off, unsigned n_images, uint64_t total,
                                                       const int *__restrict__ track, const unsigned *__restrict__ len,
                                                       unsigned *__restrict__ dup) {
    __shared__ __attribute__((aligned(16))) int s_label[kDupTile];
    const uint64_t slot = blockIdx.x;
    auto start = [&](unsigned m) { return (image_off[m] < total ? image_off[m] : total) / kDupTile + m; };
    const unsigned m = last_pair_at_or_before(n_images, slot, start);
    long first, n;
    image_rows(image_off, n_images, total, m, first, n);
    const long block = (long)slot - (first / kDupTile + (long)m);
    if (block < 0) return;                                       // rows in front of the first image
    const long r0 = block * kDupTile;
    if (r0 >= n) return;                                         // the image's idle slot(s)
    const int tid = threadIdx.x;
    const bool on = r0 + tid < n;
    const int mine = on ? track[first + r0 + tid] : -1;
    bool open = on && !(len && len[mine] == 1u), hit = false;
    for (long t0 = 0; t0 <= r0; t0 += kDupTile) {                // (the same for the whole workgroup)
        __syncthreads();                                         // everybody is done with the tile before
        s_label[tid] = t0 + tid < n ? track[first + t0 + tid] : -1;
        __syncthreads();
        if (__ballot(open) == 0) continue;                       // (wave-uniform)
        bool found = false;
        if (t0 < r0) {                                           // a tile in front: every label of it (wave-uniform)
#pragma unroll 4
            for (int i = 0; i < kDupTile; i += 4) {
                const int4 l = *reinterpret_cast<const int4 *>(s_label + i);
                found |= (l.x == mine) | (l.y == mine) | (l.z == mine) | (l.w == mine);
            }
        } else {                                                 // its own tile: a row looks at the rows below it only
#pragma unroll 4
            for (int i = 0; i < kDupTile; i += 4) {
                const int4 l = *reinterpret_cast<const int4 *>(s_label + i);
                found |= (l.x == mine && i < tid) | (l.y == mine && i + 1 < tid) | (l.z == mine && i + 2 < tid) |
                         (l.w == mine && i + 3 < tid);
            }
        }
        if (open && found) {
            hit = true;
            open = false;
        }
    }
    count_label(dup, mine, hit);
}

unsigned build_tracks_link_entries() { return kLinkEntries; }
unsigned build_tracks_dup_tile() { return kDupTile; }

void launch_build_tracks(const uint64_t *image_off, unsigned n_images, uint64_t total, const unsigned *edge_a,
                         const unsigned *edge_b, const uint64_t *edge_off, uint64_t capacity, unsigned n_edges, const int *match,
                         bool accumulate, int *track, unsigned *len, unsigned *dup, hipStream_t stream) {
    if (total == 0) return;
    const long n = (long)total;
    const unsigned row_blocks = (unsigned)((n + kRowThreads - 1) / kRowThreads);
    if (!accumulate) hipLaunchKernelGGL(tracks_init, dim3(row_blocks), dim3(kRowThreads), 0, stream, track, n);
    if (n_edges)
        hipLaunchKernelGGL(tracks_link, dim3((unsigned)(capacity / kLinkEntries + n_edges)), dim3(kLinkEntries), 0, stream,
                           image_off, n_images, total, edge_a, edge_b, edge_off, capacity, n_edges, match, track);
    hipLaunchKernelGGL(tracks_flatten, dim3(row_blocks), dim3(kRowThreads), 0, stream, track, n);
    if (!len && !dup) return;
    hipLaunchKernelGGL(tracks_zero, dim3(row_blocks), dim3(kRowThreads), 0, stream, len, dup, n);
    if (len) hipLaunchKernelGGL(tracks_len, dim3(row_blocks), dim3(kRowThreads), 0, stream, track, n, len);
    if (dup && n_images)
        hipLaunchKernelGGL(tracks_dup, dim3((unsigned)(total / kDupTile + n_images)), dim3(kDupTile), 0, stream, image_off,
                           n_images, total, track, len, dup);
}

}  // namespace lfmkd
