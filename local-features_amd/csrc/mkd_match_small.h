// The one-launch ("small") matcher's workgroup body and the batched form's pair arithmetic, shared by mkd_match.hip
// (match_small, match_small_both, match_small_pairs) and mkd_match_guided.hip (match_small_guided_pairs): each of the two
// units compiles its own copy, no device code crosses a translation unit.  The notes on the form are in mkd_match.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace lfmkd {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

}  // namespace

constexpr int kSmallWaves = 16;

// (the body of a workgroup: `block` = which 16 rows of a it owns)
__device__ __forceinline__ void match_small_block(const float *__restrict__ a, long na, const float *__restrict__ b, long nb,
                                                  const unsigned *__restrict__ excl_lo, const unsigned *__restrict__ excl_hi,
                                                  float ratio, int *__restrict__ match, float *__restrict__ best_out,
                                                  float *__restrict__ second_out, long block) {
    __shared__ float s_best[kSmallWaves][16], s_second[kSmallWaves][16];
    __shared__ int s_idx[kSmallWaves][16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 15, g = lane >> 4;
    const long arow = block * 16 + n;
    const long arow_c = arow < na ? arow : na - 1;
    struct Raw { f32x4 v[8]; };   // a row's share of the four k-steps: k = 32 s + 8 g .. + 7
    auto load_row = [&](const float *row) {
        Raw r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            r.v[2 * s] = *reinterpret_cast<const f32x4 *>(row + 32 * s + 8 * g);
            r.v[2 * s + 1] = *reinterpret_cast<const f32x4 *>(row + 32 * s + 8 * g + 4);
        }
        return r;
    };
    float one = 1.f;
    asm("" : "+v"(one));   // (keeps the residual a single v_fma_mix_f32: see AFrag in mkd_describe.hip)
    auto split8 = [&](const f32x4 &v0, const f32x4 &v1, h8 &hi, h8 &lo) {
        const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        u32x4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(v[2 * e], v[2 * e + 1]));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float r0 = __builtin_fmaf(v[2 * e], one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(h[e] & 0xffffu)));
            const float r1 = __builtin_fmaf(v[2 * e + 1], one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(h[e] >> 16)));
            l[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
        }
        hi = __builtin_bit_cast(h8, h);
        lo = __builtin_bit_cast(h8, l);
    };
    const long b_tiles = (nb + 15) / 16;
    auto b_row = [&](long t) {   // as A operand: lane (n, g) brings b row n of tile t (clamped: masked below)
        const long r = t * 16 + n;
        return b + (r < nb ? r : nb - 1) * 128;
    };
    // the wave's first b tile is requested together with its a rows: one round trip to memory in front of the loop, not two
    const Raw ra = load_row(a + arow_c * 128);
    Raw cur = load_row(b_row(wave < b_tiles ? wave : 0));
    // a fragments: lane (n, g) holds a[row n][32 s + 8 g + j] of k-step s
    h8 ah[4], al[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) split8(ra.v[2 * s], ra.v[2 * s + 1], ah[s], al[s]);
    const unsigned lo_x = excl_lo && arow < na ? excl_lo[arow] : 0u, hi_x = excl_lo && arow < na ? excl_hi[arow] : 0u;
    float best = -INFINITY, second = -INFINITY;
    int best_i = -1;
    for (long t = wave; t < b_tiles; t += kSmallWaves) {
        const long tn = t + kSmallWaves < b_tiles ? t + kSmallWaves : t;
        const Raw nxt = load_row(b_row(tn));                // in flight while this tile is split and multiplied
        // (the scheduler sinks these eight requests into the tile's arithmetic -- 60 VGPRs of the 128 the launch bounds allow;
        //  fencing them here, all in flight before the tile's first instruction at 127 VGPRs, was measured in round 5 and is
        //  SLOWER: 2000 x 2000 38 us instead of 35, 500 x 500 17 instead of 14)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            h8 bh, bl;
            split8(cur.v[2 * s], cur.v[2 * s + 1], bh, bl);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, ah[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, al[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, ah[s], acc, 0, 0, 0);
        }
        // the lane holds (a row n) x (b rows 16 t + 4 g + i), ascending: the later index wins among equals.  (The scan's
        // "does this tile hold a new best at all" short cut was measured here and lost 3 us at 2000 x 2000: with eight tiles
        // per wave the running best is still settling in most of them.)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned row = (unsigned)(t * 16 + 4 * g + i);
            const bool masked = row >= (unsigned)nb || (row >= lo_x && row < hi_x);
            const float v = masked ? -INFINITY : acc[i];
            const bool nb_ = v >= best && v > -INFINITY;
            const bool ns = !nb_ && v > second;
            second = nb_ ? best : (ns ? v : second);
            best_i = nb_ ? (int)row : best_i;
            best = nb_ ? v : best;
        }
        cur = nxt;
    }
    // fold: the four row groups of a column (lanes n, n + 16, n + 32, n + 48), then the waves
    auto fold = [](float &b0, int &i0, float &s0, float ob, int oi, float os) {
        const bool other = ob > b0 || (ob == b0 && oi > i0);
        const float ns = other ? fmaxf(b0, os) : fmaxf(s0, ob);
        i0 = other ? oi : i0;
        b0 = other ? ob : b0;
        s0 = ns;
    };
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {
        const float ob = __shfl_xor(best, m), os = __shfl_xor(second, m);
        const int oi = __shfl_xor(best_i, m);
        fold(best, best_i, second, ob, oi, os);
    }
    if (g == 0) { s_best[wave][n] = best; s_second[wave][n] = second; s_idx[wave][n] = best_i; }
    __syncthreads();
    float bb = -INFINITY, ss = -INFINITY;
    int bi = -1;
    if (threadIdx.x < 16) {
        bb = s_best[0][n];
        ss = s_second[0][n];
        bi = s_idx[0][n];
#pragma unroll
        for (int w = 1; w < kSmallWaves; ++w) fold(bb, bi, ss, s_best[w][n], s_idx[w][n], s_second[w][n]);
    }
    if (threadIdx.x < 16 && arow < na) {
        match[arow] = (bi >= 0 && (ratio <= 0.f || bb * ratio > ss)) ? bi : -1;
        if (best_out) best_out[arow] = bb;
        if (second_out) second_out[arow] = ss;
    }
}

// the first row and the number of rows of a pair whose two offsets are first and next
__device__ __forceinline__ void pair_rows(uint64_t first, uint64_t next, uint64_t total, long &lo, long &n) {
    const uint64_t o0 = first < total ? first : total, o1 = next < total ? next : total;
    lo = (long)o0;
    n = o1 > o0 ? (long)(o1 - o0) : 0;
}

// the first row and the number of rows of image m of a pool; an id at or beyond n_images names an empty image
__device__ __forceinline__ void image_rows(const uint64_t *__restrict__ image_off, unsigned n_images, uint64_t total, unsigned m,
                                           long &lo, long &n) {
    lo = 0;
    n = 0;
    if (m < n_images) pair_rows(image_off[m], image_off[m + 1], total, lo, n);
}

// the largest p of [0, n_pairs) with key(p) <= v, for a strictly or weakly increasing key; n_pairs > 0 (the caller checks
// key(p) <= v itself: v may lie in front of pair 0)
template <typename Key>
__device__ __forceinline__ unsigned last_pair_at_or_before(unsigned n_pairs, uint64_t v, Key key) {
    unsigned lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (key(mid) <= v) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace lfmkd
