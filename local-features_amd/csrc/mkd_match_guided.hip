// gfx950 guided matching (lf_mkd_match_guided_pairs_device, include/lf_mkd.h): the batched pair matcher of mkd_match.hip
// once more, with each row's candidates restricted to the rows of the other side that the pair's verified model allows --
// a transfer disc under a homography, an epipolar band under a fundamental matrix.
//
// `match_small_guided_pairs` has match_small_pairs' slot map and workgroup shape (mkd_match_small.h: 16 rows of x per
// workgroup -- x = a in the a -> b direction, b in the other --, 16 waves taking the 16-row tiles of y round-robin) and its
// arithmetic for a tile: the same split, the same three terms in the same order, the same top-2 update and folds.  What it
// adds sits IN FRONT of a tile: lane (n, g) holds the keypoint of x row n and tests it against the keypoints of its four y
// rows 16 t + 4 g + i (8 bytes per row instead of a descriptor's 512); a wave-wide vote then decides whether the tile is
// run at all.  A tile without an admissible pair costs no descriptor request, no split and no MFMA; in a tile that is run
// the inadmissible pairs are masked in the top-2 update, as rows beyond the pair's end always were.  The vote for a
// wave's next tile is taken before that tile's descriptor rows are requested, so the one-tile-ahead prefetch of the body
// only ever fetches tiles that will be used.  The y side's keypoints are staged in LDS by the whole workgroup, 4096 rows
// (32 KiB) at a time: read from memory per tile they cost every skipped tile a round trip of its own, and a wave whose
// tiles are all skipped -- the ordinary case under a homography -- did nothing but wait for them (measured: 128 pairs of
// 2000 x 2000 under H in 1756 us that way).
//
// The admissibility test is the verifiers' inlier test, op for op (mkd_guided_math.h), with the model's nine floats in
// scalar registers; both directions evaluate pred(a_i, b_j) -- the reverse direction exchanges the operands' roles, not the
// predicate's arguments -- so the relation is symmetric by construction and LF_MKD_MATCH_MUTUAL means what it says.
//
// Contraction: mkd_guided_math.h switches contraction off for the rest of this unit, as the verifiers' units are built; the
// similarity's arithmetic is MFMAs and one explicit fma per element, to which the mode makes no difference.  The unguided
// kernels live in mkd_match.hip and keep the mode they are built with.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_match_small.h"

#include "mkd_guided_math.h"   // (last: its file-scope pragma holds from here on)

namespace lfmkd {
namespace {

// MODE = 2 kind + rev.  What a lane keeps of its own x row, and the test of a y row's keypoint (qx, qy) against it.
template <int MODE>
struct Guide;
template <>
struct Guide<0> {   // homography, x = a: the mapped point is the row's
    GuideHA a;
    __device__ __forceinline__ Guide(const float *m, float px, float py, float thr2) : a(guide_h_of_a(m, px, py, thr2)) {}
    __device__ __forceinline__ bool test(const float *, float qx, float qy, float) const { return guide_h_test(a, qx, qy); }
};
template <>
struct Guide<1> {   // homography, x = b: every y row is mapped
    float bx, by;
    __device__ __forceinline__ Guide(const float *, float px, float py, float) : bx(px), by(py) {}
    __device__ __forceinline__ bool test(const float *m, float qx, float qy, float thr2) const {
        return guide_h_test(guide_h_of_a(m, qx, qy, thr2), bx, by);
    }
};
template <>
struct Guide<2> {   // fundamental matrix, x = a: the row's epipolar line
    GuideFA a;
    __device__ __forceinline__ Guide(const float *m, float px, float py, float) : a(guide_f_of_a(m, px, py)) {}
    __device__ __forceinline__ bool test(const float *m, float qx, float qy, float thr2) const {
        return guide_f_test(a, guide_f_of_b(m, qx, qy), thr2);
    }
};
template <>
struct Guide<3> {   // fundamental matrix, x = b
    GuideFB b;
    __device__ __forceinline__ Guide(const float *m, float px, float py, float) : b(guide_f_of_b(m, px, py)) {}
    __device__ __forceinline__ bool test(const float *m, float qx, float qy, float thr2) const {
        return guide_f_test(guide_f_of_a(m, qx, qy), b, thr2);
    }
};

constexpr int kKpChunk = 4096;   // y rows whose keypoints sit in LDS at a time: 32 KiB, 256 tiles, 16 per wave
struct SmallShared {
    float best[kSmallWaves][16], second[kSmallWaves][16];
    int idx[kSmallWaves][16];
    float2 kp[kKpChunk];
};

// The body of a workgroup: match_small_block (mkd_match_small.h) over x [nx][128] against y [ny][128] with the vote in front
// of every tile.  kx / ky: the two sides' keypoints (rows of 5 floats), m: the pair's model.  ny may be 0 or 1.
template <int MODE>
__device__ __forceinline__ void guided_block(const float *__restrict__ x, const float *__restrict__ kx, long nx,
                                             const float *__restrict__ y, const float *__restrict__ ky, long ny,
                                             const float *__restrict__ m, float thr2, float ratio, int *__restrict__ match,
                                             float *__restrict__ best_out, float *__restrict__ second_out, long block,
                                             SmallShared &sh) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 15, g = lane >> 4;
    const long xrow = block * 16 + n;
    const long xrow_c = xrow < nx ? xrow : nx - 1;
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
    auto y_row = [&](long t) {   // as A operand: lane (n, g) brings y row n of tile t (clamped: masked below)
        const long r = t * 16 + n;
        return y + (r < ny ? r : ny - 1) * 128;
    };
    float best = -INFINITY, second = -INFINITY;
    int best_i = -1;
    // the x row and its share of the predicate: requested in front of the first barrier, in flight beside the staging below
    const Raw rx = load_row(x + xrow_c * 128);
    const Guide<MODE> mine(m, kx[xrow_c * 5], kx[xrow_c * 5 + 1], thr2);
    // x fragments: lane (n, g) holds x[row n][32 s + 8 g + j] of k-step s
    h8 xh[4], xl[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) split8(rx.v[2 * s], rx.v[2 * s + 1], xh[s], xl[s]);
    // y in chunks of kKpChunk rows (one chunk for any pair the call is meant for): the workgroup stages the chunk's
    // keypoints in LDS -- one round trip to memory for all of them, not one per tile and wave -- and every wave then walks
    // its tiles of the chunk.  The chunk loop and its barriers are the same for every wave of the workgroup.
    for (long c0 = 0; c0 < ny; c0 += kKpChunk) {
        const long cn = ny - c0 < kKpChunk ? ny - c0 : kKpChunk;
        if (c0) __syncthreads();                             // the previous chunk's keypoints have been read
        for (long i = threadIdx.x; i < cn; i += 64 * kSmallWaves) sh.kp[i] = make_float2(ky[(c0 + i) * 5], ky[(c0 + i) * 5 + 1]);
        __syncthreads();
        const long t_end = (c0 + cn + 15) / 16;              // the chunk's tiles: [c0 / 16, t_end), c0 / 16 a multiple of 16
        // From tile t on, the wave's next tile of the chunk with an admissible pair and the lane's four bits of it (a row
        // at or beyond ny is never admissible: its keypoint is read as the chunk's last).  The vote is over the whole wave:
        // every branch on it is wave-uniform.
        auto next_used = [&](long &t, unsigned &adm) {
            for (; t < t_end; t += kSmallWaves) {
                adm = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long r = t * 16 + 4 * g + i;
                    const float2 q = sh.kp[(r < ny ? r : ny - 1) - c0];
                    const bool ok = mine.test(m, q.x, q.y, thr2) && r < ny && xrow < nx;
                    adm |= ok ? 1u << i : 0u;
                }
                if (__builtin_amdgcn_ballot_w64(adm != 0u) != 0ull) return true;
            }
            return false;
        };
        long t = c0 / 16 + wave;
        unsigned adm = 0u;
        bool have = next_used(t, adm);
        if (!have) continue;                                 // (wave-uniform; the barriers are at the head of the loop)
        Raw cur = load_row(y_row(t));
        while (have) {
            long tn = t + kSmallWaves;
            unsigned adm_n = 0u;
            const bool have_n = next_used(tn, adm_n);   // the vote first: only a tile that will be run is requested
            // in flight while this tile is split and multiplied (after the last tile: this tile once more, as match_small_block
            // does -- a branch around the request would keep all of it in registers beside all of `cur`)
            const Raw nxt = load_row(y_row(have_n ? tn : t));
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                h8 yh, yl;
                split8(cur.v[2 * s], cur.v[2 * s + 1], yh, yl);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(yl, xh[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(yh, xl[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(yh, xh[s], acc, 0, 0, 0);
            }
            // the lane holds (x row n) x (y rows 16 t + 4 g + i), ascending: the later index wins among equals
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned row = (unsigned)(t * 16 + 4 * g + i);
                const bool masked = !((adm >> i) & 1u);   // (a row at or beyond ny is never admissible)
                const float v = masked ? -INFINITY : acc[i];
                const bool nb_ = v >= best && v > -INFINITY;
                const bool ns = !nb_ && v > second;
                second = nb_ ? best : (ns ? v : second);
                best_i = nb_ ? (int)row : best_i;
                best = nb_ ? v : best;
            }
            cur = nxt;
            t = tn;
            adm = adm_n;
            have = have_n;
        }
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
    for (int w = 16; w <= 32; w <<= 1) {
        const float ob = __shfl_xor(best, w), os = __shfl_xor(second, w);
        const int oi = __shfl_xor(best_i, w);
        fold(best, best_i, second, ob, oi, os);
    }
    if (g == 0) { sh.best[wave][n] = best; sh.second[wave][n] = second; sh.idx[wave][n] = best_i; }
    __syncthreads();
    float bb = -INFINITY, ss = -INFINITY;
    int bi = -1;
    if (threadIdx.x < 16) {
        bb = sh.best[0][n];
        ss = sh.second[0][n];
        bi = sh.idx[0][n];
#pragma unroll
        for (int w = 1; w < kSmallWaves; ++w) fold(bb, bi, ss, sh.best[w][n], sh.idx[w][n], sh.second[w][n]);
    }
    if (threadIdx.x < 16 && xrow < nx) {
        match[xrow] = (bi >= 0 && (ratio <= 0.f || bb * ratio > ss)) ? bi : -1;
        if (best_out) best_out[xrow] = bb;
        if (second_out) second_out[xrow] = ss;
    }
}

}  // namespace

// One direction (slots_ab workgroups, match_ba == nullptr) or both, found as match_small_pairs finds them.  There is no
// refusal of a small side here: a pair's one row is a legitimate candidate set, and an empty side leaves -1 / -inf.
__global__ __launch_bounds__(64 * kSmallWaves) void match_small_guided_pairs(
    const float *__restrict__ a, const float *__restrict__ kps_a, const uint64_t *__restrict__ off_a, uint64_t na_total,
    const float *__restrict__ b, const float *__restrict__ kps_b, const uint64_t *__restrict__ off_b, uint64_t nb_total,
    const float *__restrict__ model, unsigned n_pairs, unsigned slots_ab, unsigned kind, float thr2, float ratio,
    int *__restrict__ match_ab, int *__restrict__ match_ba, float *__restrict__ best_out, float *__restrict__ second_out) {
    __shared__ SmallShared sh;
    const bool rev = blockIdx.x >= slots_ab;
    const uint64_t slot = rev ? blockIdx.x - slots_ab : blockIdx.x;
    const uint64_t *off_x = rev ? off_b : off_a, *off_y = rev ? off_a : off_b;
    const uint64_t x_total = rev ? nb_total : na_total, y_total = rev ? na_total : nb_total;
    auto start = [&](unsigned p) { return (off_x[p] < x_total ? off_x[p] : x_total) / 16 + p; };
    const unsigned p = last_pair_at_or_before(n_pairs, slot, start);
    uint64_t x0 = off_x[p], x1 = off_x[p + 1], y0 = off_y[p], y1 = off_y[p + 1];
    asm volatile("" : "+s"(x0), "+s"(x1), "+s"(y0), "+s"(y1));   // (requested together: see match_small_pairs)
    long x_lo, nx, y_lo, ny;
    pair_rows(x0, x1, x_total, x_lo, nx);
    pair_rows(y0, y1, y_total, y_lo, ny);
    const long block = (long)slot - (x_lo / 16 + (long)p);   // slot - start(p)
    if (block < 0) return;                             // rows in front of the first pair
    if (block * 16 >= nx) return;                      // the pair's idle slot(s)
    int *match = (rev ? match_ba : match_ab) + x_lo;
    float *best = rev || !best_out ? nullptr : best_out + x_lo, *second = rev || !second_out ? nullptr : second_out + x_lo;
    const float *m = model + 9 * (size_t)p;
    const float *x = (rev ? b : a) + x_lo * 128, *y = (rev ? a : b) + y_lo * 128;
    const float *kx = (rev ? kps_b : kps_a) + x_lo * 5, *ky = (rev ? kps_a : kps_b) + y_lo * 5;
    // (kind and rev are the same for the whole workgroup: a scalar branch)
    if (kind == 0u) {
        if (!rev) guided_block<0>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best, second, block, sh);
        else guided_block<1>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best, second, block, sh);
    } else {
        if (!rev) guided_block<2>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best, second, block, sh);
        else guided_block<3>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best, second, block, sh);
    }
}

void launch_match_guided_pairs(const float *a, const float *kps_a, const uint64_t *off_a, uint64_t na_total, const float *b,
                               const float *kps_b, const uint64_t *off_b, uint64_t nb_total, const float *model,
                               unsigned n_pairs, unsigned kind, float threshold, float ratio, bool mutual, int *match_ab,
                               int *match_ba, float *best, float *second, hipStream_t stream) {
    if (n_pairs == 0) return;
    const float thr2 = threshold * threshold;   // as launch_verify and launch_fundamental form it
    const uint64_t slots_ab = match_pairs_slots(na_total, n_pairs);
    const uint64_t slots = slots_ab + (match_ba ? match_pairs_slots(nb_total, n_pairs) : 0);
    hipLaunchKernelGGL(match_small_guided_pairs, dim3((unsigned)slots), dim3(64 * kSmallWaves), 0, stream, a, kps_a, off_a,
                       na_total, b, kps_b, off_b, nb_total, model, n_pairs, (unsigned)slots_ab, kind, thr2, ratio, match_ab,
                       match_ba, best, second);
    if (mutual) launch_match_mutual(off_a, na_total, off_b, nb_total, n_pairs, match_ab, match_ba, stream);
}

}  // namespace lfmkd
