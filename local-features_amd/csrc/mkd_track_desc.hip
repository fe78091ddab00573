// gfx950 track descriptors (include/lf_mkd.h, lf_mkd_track_descriptors_device): per track of a track table ONE
// 8-bit row -- the sum of its observations' centred pool rows, normalised and quantised again -- so that a reconstruction
// carries descriptors of its own and lf_mkd_match_q8_device against them gives the d_row_track that resection reads.  The
// arithmetic is csrc/mkd_track_desc_math.h, which the host twin compiles too.
//
//   track_descriptors<G>  ONE launch.  A GROUP of G = 8 lanes owns a track and a lane 128 / G = 16 bytes of the row: 8 tracks a
//                         wave, 32 a workgroup, and a contributor's row is one 128-byte request of the group.  The walk takes
//                         kAhead = 4 positions a step: their obs_row (and state) loads are issued first, then the rows', then
//                         the bytes are added to 16 integer accumulators a lane (sums of RAW bytes; 128 C comes off once, at
//                         the end).  n2 is a butterfly over lane xor 4, 2, 1 of int64 partial sums; the quantiser is f64.
//                         With d_desc_stats a second walk over the same rows (L2-warm) forms each contributor's similarity
//                         with the quantised row (a butterfly a contributor) and keeps the smallest.
//                         LONG TRACKS: a track of more than kTdLong = 256 positions is left out of its group's walk and taken
//                         by the WHOLE WAVE, one such track at a time: group g walks positions lo + g, lo + g + 8, .., the
//                         groups' sums combine by a butterfly over lane xor 8, 16, 32, and the owning group goes on with the
//                         totals.  Integer sums: the order changes nothing.  (G = 4 and G = 16 are compiled too, for
//                         LF_MKD_TRACK_DESC_LANES in the environment: the A/B of profiles/track_descriptors.md, same bits.)
//
// No scratch memory, no LDS, no allocation, no atomic, and no workgroup waits for another.  Every loop that holds a lane
// permute runs in wave-uniform control flow: its condition is an __any or a ballot's bits, and a group that is done goes
// through the steps with its predicate off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "mkd_device.h"
#include "mkd_track_desc_math.h"
#include "mkd_scene.h"   // behind the arithmetic, as in the other reconstruction stages

namespace lfmkd {
namespace {

constexpr int kThreads = kSumThreads;
constexpr unsigned kMaxBlocks = 16384;                  // grid-stride beyond
constexpr int kAhead = 4;                               // positions whose loads are issued before the first is consumed
constexpr unsigned kTdLong = 256;                       // a track of more positions is walked by the whole wave

struct TdArgs {
    SceneTables tb;
    const unsigned char *__restrict__ q;
    const unsigned *__restrict__ obs_state;
    unsigned min_state;
    const float *__restrict__ points;
    double cmin, scale;
    unsigned char *__restrict__ desc;
    int *__restrict__ stats;
};

// a lane's W words of a row
template <int W>
struct Piece {
    uint32_t w[W];
};
template <int W>
__device__ __forceinline__ Piece<W> load_piece(const unsigned char *p) {
    Piece<W> r;
    if constexpr (W == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        r.w[0] = v.x, r.w[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < W / 4; ++i) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            r.w[4 * i] = v.x, r.w[4 * i + 1] = v.y, r.w[4 * i + 2] = v.z, r.w[4 * i + 3] = v.w;
        }
    }
    return r;
}
template <int W>
__device__ __forceinline__ void store_piece(unsigned char *p, const Piece<W> &r) {
    if constexpr (W == 2) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(r.w[0], r.w[1]);
    } else {
#pragma unroll
        for (int i = 0; i < W / 4; ++i)
            reinterpret_cast<uint4 *>(p)[i] = make_uint4(r.w[4 * i], r.w[4 * i + 1], r.w[4 * i + 2], r.w[4 * i + 3]);
    }
}

// The positions first, first + step, .. below hi of the observation arrays, kAhead a step, lane l of its group.
//   kSpread false: C counts the contributors, and with `rows` their raw bytes are added to acc.
//   kSpread true:  acc holds the quantised row's q; spread goes down to the smallest similarity of a contributor with it.
// Wave-uniform: called by every lane, with hi <= first for a group that has nothing to walk.  last = O - 1: the index and state
// loads of a position at or beyond hi go there instead (every hi is at most O), and what they return is not looked at.
template <int G, bool kSpread>
__device__ __forceinline__ void td_walk(const TdArgs &a, uint64_t last, uint64_t first, uint64_t step, uint64_t hi, bool rows, unsigned l,
                                        unsigned &C, int (&acc)[kTdRow / G], int &spread) {
    constexpr int B = kTdRow / G, W = B / 4;
    const unsigned *__restrict__ states = a.obs_state ? a.obs_state : reinterpret_cast<const unsigned *>(a.tb.obs_row);
    for (uint64_t k0 = first; __any(k0 < hi); k0 += kAhead * step) {
        // Three phases without a branch between their loads.  Every lane loads at every position: an index and a state from
        // a position that exists (some lane has k0 < hi <= O, so last = O - 1 does; the state from the index array where there
        // is no state array), and a row from row 0 where it has no contributor (a walk only steps in a pool of at least one
        // row: launch_track_descriptors).  What such a load returns is masked out.
        int row[kAhead];
        unsigned st[kAhead];
        bool ok[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const uint64_t k = k0 + u * step, kk = k < last ? k : last;
            row[u] = a.tb.obs_row[kk];
            st[u] = states[kk];
        }
        Piece<W> p[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            ok[u] = (k0 + u * step < hi) & td_contributes(a.obs_state != nullptr, st[u], a.min_state, row[u], a.tb.n_rows);
            p[u] = load_piece<W>(a.q + (uint64_t)((ok[u] & rows) ? row[u] : 0) * kTdRow + l * B);
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
#pragma unroll
            for (int i = 0; i < W; ++i) p[u].w[i] = (ok[u] & rows) ? p[u].w[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if constexpr (!kSpread) {
                C += ok[u] ? 1u : 0u;
#pragma unroll
                for (int j = 0; j < B; ++j) acc[j] += (int)((p[u].w[j / 4] >> (8 * (j % 4))) & 0xFFu);   // (a zero piece adds nothing)
            } else {
                int d = 0;
#pragma unroll
                for (int j = 0; j < B; ++j) d += td_term((p[u].w[j / 4] >> (8 * (j % 4))) & 0xFFu, acc[j]);
#pragma unroll
                for (int m = G / 2; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
                spread = ok[u] && d < spread ? d : spread;
            }
        }
    }
}

}  // namespace

template <int G>
__global__ __launch_bounds__(kThreads) void track_descriptors(TdArgs a) {
    constexpr int B = kTdRow / G, W = B / 4, kGroups = 64 / G;
    const uint64_t T = clamp_to(a.tb.counts[0], a.tb.tcap), O = clamp_to(a.tb.counts[1], a.tb.ocap);
    const uint64_t last = O ? O - 1 : 0;                                          // (with O == 0 no walk takes a step)
    const unsigned lane = threadIdx.x & 63, l = lane & (G - 1), base = lane & ~(unsigned)(G - 1), grp = lane / G;
    const uint64_t first = ((uint64_t)blockIdx.x * kSumWaves + (threadIdx.x >> 6)) * kGroups;
    const uint64_t stride = (uint64_t)gridDim.x * kSumWaves * kGroups;
    for (uint64_t t0 = first; t0 < a.tb.tcap; t0 += stride) {                    // wave-uniform
        const uint64_t t = t0 + grp;
        const bool alive = t < T;
        uint64_t lo = 0, hi = 0;
        if (alive) track_range(a.tb, t, O, lo, hi);
        hi = hi - lo > kTdMaxObs ? lo + kTdMaxObs : hi;
        const bool described = alive && td_described(a.points, t, a.cmin);
        if (!described && !a.stats) hi = lo;                                      // nothing of it is asked for
        const bool is_long = hi - lo > kTdLong;

        // the contributors' number and the sums of their raw bytes
        unsigned C = 0;
        int acc[B], none = 0;
#pragma unroll
        for (int j = 0; j < B; ++j) acc[j] = 0;
        td_walk<G, false>(a, last, lo, 1, is_long ? lo : hi, described, l, C, acc, none);
        for (uint64_t todo = __ballot(is_long); todo;) {                          // wave-uniform: one long track at a time
            const int src = __ffsll((unsigned long long)todo) - 1;               // its group's first lane
            todo &= ~(((1ull << G) - 1ull) << src);
            const uint64_t flo = __shfl((unsigned long long)lo, src, 64), fhi = __shfl((unsigned long long)hi, src, 64);
            const bool frows = __shfl((int)described, src, 64) != 0;
            unsigned fC = 0;
            int facc[B];
#pragma unroll
            for (int j = 0; j < B; ++j) facc[j] = 0;
            td_walk<G, false>(a, last, flo + grp, kGroups, fhi, frows, l, fC, facc, none);
#pragma unroll
            for (int m = G; m < 64; m <<= 1) {
                fC += __shfl_xor(fC, m, 64);
#pragma unroll
                for (int j = 0; j < B; ++j) facc[j] += __shfl_xor(facc[j], m, 64);
            }
            if (base == (unsigned)src) {
                C = fC;
#pragma unroll
                for (int j = 0; j < B; ++j) acc[j] = facc[j];
            }
        }

        // S, n2, the quantised row
        int S[B], q[B];
        long long n2 = 0;
#pragma unroll
        for (int j = 0; j < B; ++j) {
            S[j] = td_centre((uint32_t)acc[j], C);
            n2 += td_square(S[j]);
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m, 64);
        const bool full = described && C > 0 && n2 > 0;
        const double norm = td_norm(full ? n2 : 1);
#pragma unroll
        for (int j = 0; j < B; ++j) q[j] = full ? td_quantize(S[j], a.scale, norm) : 0;

        // the second walk: the smallest similarity of a contributor with the row
        int spread = kTdNoSpread;
        if (a.stats) {                                                            // wave-uniform
            int s = INT32_MAX;
            unsigned unused = 0;
            td_walk<G, true>(a, last, lo, 1, full && !is_long ? hi : lo, true, l, unused, q, s);
            for (uint64_t todo = __ballot(is_long && full); todo;) {
                const int src = __ffsll((unsigned long long)todo) - 1;
                todo &= ~(((1ull << G) - 1ull) << src);
                const uint64_t flo = __shfl((unsigned long long)lo, src, 64), fhi = __shfl((unsigned long long)hi, src, 64);
                int fq[B], fs = INT32_MAX;
#pragma unroll
                for (int j = 0; j < B; ++j) fq[j] = __shfl(q[j], src + (int)l, 64);
                td_walk<G, true>(a, last, flo + grp, kGroups, fhi, true, l, unused, fq, fs);
#pragma unroll
                for (int m = G; m < 64; m <<= 1) {
                    const int other = __shfl_xor(fs, m, 64);
                    fs = other < fs ? other : fs;
                }
                if (base == (unsigned)src) s = fs;
            }
            spread = full ? s : kTdNoSpread;
        }

        if (t < a.tb.tcap) {                                                      // T .. tcap - 1: zero rows too
            Piece<W> out;
#pragma unroll
            for (int i = 0; i < W; ++i)
                out.w[i] = (uint32_t)(q[4 * i] + 128) | (uint32_t)(q[4 * i + 1] + 128) << 8 | (uint32_t)(q[4 * i + 2] + 128) << 16 |
                           (uint32_t)(q[4 * i + 3] + 128) << 24;
            store_piece<W>(a.desc + t * kTdRow + l * B, out);
            if (a.stats && l == 0) {
                a.stats[2 * t] = (int)C;
                a.stats[2 * t + 1] = spread;
            }
        }
    }
}

namespace {
template <int G>
void launch_form(const TdArgs &a, hipStream_t stream) {
    const uint64_t per_block = kThreads / G, want = (a.tb.tcap + per_block - 1) / per_block;
    hipLaunchKernelGGL(track_descriptors<G>, dim3((unsigned)(want < kMaxBlocks ? want : kMaxBlocks)), dim3(kThreads), 0, stream, a);
}
}  // namespace

void launch_track_descriptors(const SceneTables &tb, const unsigned char *q, const unsigned *obs_state, unsigned min_state,
                              const float *points, double cmin, float scale, unsigned char *desc, int *stats, hipStream_t stream) {
    if (tb.tcap == 0) return;
    TdArgs a = {tb, q, obs_state, min_state, points, cmin, double(scale), desc, stats};
    if (tb.n_rows == 0) a.tb.ocap = 0;      // no row, no contributor: the walks take no step, and none ever reads a row of an empty pool
    // LF_MKD_TRACK_DESC_LANES=4 / 16 in the environment (read per launch): the other group widths, for A/B runs; same bits
    const char *e = getenv("LF_MKD_TRACK_DESC_LANES");
    const int lanes = e ? atoi(e) : 8;
    if (lanes == 4) launch_form<4>(a, stream);
    else if (lanes == 16) launch_form<16>(a, stream);
    else launch_form<8>(a, stream);
}

}  // namespace lfmkd
