// MKD descriptor path, the describe kernel: device code for gfx950 (CDNA4, wave64).
//
//   mkd_pool   mkd/patch_gradients.glsl:72-104 + mkd/embedding.glsl:53-121 (both variants)
//              + mkd/normalize.glsl:22-142 + mkd/whitening.glsl:22-77 + mkd/normalize_final.glsl
// (paths under local_features/src/vulkan/shaders/; the other stages live in mkd_pyramid.hip -- pyramid and patch
//  sampling --, mkd_orient.hip, mkd_detect.hip and mkd_match.hip)
//
// Pooling is a GEMM with M = patches, K = pixels, N = (stream, spatial kernel) columns.  One wave
// owns 16 patches; lane l = (patch p = l & 15, segment q = l >> 4) holds 8 pixels of the current patch row: the block
// x in [4q, 4q+4) and its mirror image [28-4q, 32-4q), so that the row can be FOLDED about its middle inside the lane (every
// LUT column is even or odd in x: mkd_consts.hpp) -- the folded values' K slots are exactly the operand lane map of the
// 16x16 MFMAs (column = l & 15, k-group = l >> 4).  So blur, gradients and the von-Mises
// embedding are computed in the registers that feed the matrix cores; nothing but the final
// sums leaves the wave.  Horizontal neighbours come from lanes l -/+ 16 via ds_bpermute (patch mode in LF_POOL_F16X3: via
// records in a per-wave LDS area, halo_records); vertical neighbours from a ring of raw patch rows that LDS-DMA keeps filled.
// (LF_POOL_F16_FP6, an experiment frozen as a mode, keeps the earlier unfolded form: x in [8q, 8q+8) per lane.)
// LF_POOL_F16X3 leaves three of the 211 LUT columns to the vector ALU: the x-odd cartesian kernels are a product fx(x) gy_b(y),
// so their 21 packed columns cost ~40 f32 instructions per row instead of 21 matrix instructions (valu_odd_cart below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mkd_ablate.h"
#include "mkd_device.h"
#include "mkd_sample.h"

namespace lfmkd {


namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// Two adjacent pixels per register pair: arithmetic on f32x2 compiles to v_pk_{mul,add,fma}_f32, which issue
// in the time of one scalar-f32 VALU instruction (tools/micro/valu_rate.hip) -- the kernel is VALU-issue-bound.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk_set(float v) { return f32x2{v, v}; }

// LF_POOL_F16X3 and LF_POOL_F16_FP6 share everything but the arithmetic of the harmonics' cross terms (row images by
// LDS-DMA, counted vmcnt waits, the f16x3 whitening epilogue, the m stream's three tiles)
__device__ __host__ constexpr bool f16_family(int pool) { return pool == LF_POOL_F16X3 || pool == LF_POOL_F16_FP6; }

// Seven per-pixel streams -- m, and m cos / sin (k theta) for k = 1..3 -- are pooled; the rotation by gradient_angle(px)
// that the polar kernels' streams carry (embedding.glsl:70-72) is folded into the LUT (mkd_consts.hpp).
// The folded forms (fold_form(POOL)): 12 LUT tiles per patch row -- 0-2 m | 3 + 3h + {0, 1, 2} for harmonic h = k-1 -- and 21
// accumulator tiles, which are the packed output tiles themselves: 0-2 m | 3 + 6h + 2 (LUT tile) + (0: operand U, 1: V).
// (LF_POOL_F16X3 meets LUT tiles 0 and 1 of each group only -- 42 matrix instructions per row -- and fills the accumulator
//  tiles of LUT tile 2 after the last row: valu_odd_cart.)
// The unfolded form (LF_POOL_F16_FP6):
//   LUT tiles of a patch row: 0-2 m | per harmonic h = k-1, 3 + 4h + {0: P0 = EPc[0:16], 1: Q0 = EPs[0:16],
//                                      2: R = EPc[16:25] | EC[0:7], 3: S = EPs[16:25] | EC[7:9]}
//   accumulator tiles of the row loop: 0-2 m | base 3 + 7h: cos x P0 | sin x Q0 | sin x P0 + cos x Q0 (one tile: both
//                                      products of relsin[0:16]) | cos x R | sin x R | cos x S | sin x S
//   packed output tiles after the epilogue's combine step (colmap, whitening fragments): 21, see combine_tiles.
__device__ __host__ constexpr bool fold_form(int pool) { return pool != LF_POOL_F16_FP6; }
constexpr int kTiles = 21;
constexpr int kAccTiles = 21, kUnfAccTiles = 24;
__device__ __host__ constexpr int acc_tiles(bool fold) { return fold ? kAccTiles : kUnfAccTiles; }
__device__ __host__ constexpr int lut_pieces(bool fold) { return fold ? 24 : 30; }   // 1 KiB pieces per LUT row: 2 per tile
// LF_POOL_F16X3 pools the x-odd cartesian kernels -- LUT tile 2 of each group, [0 | EC_6..8]: 3 columns of 16, half of every
// K zero -- on the vector ALU instead of the matrix cores: c_k EC_{6+b}(x, y) = c_k fx(x) gy_b(y) (mkd_consts.hpp), so per
// row and stream a lane adds gy_b(y) * sum_i fx(4q + i) s_o(4q + i) to three f32 sums, and accumulator tiles 2, 7, 8, 13, 14,
// 19, 20 are rebuilt from them once per batch (rebuild_odd_cart).  The tiles' LUT pieces are then neither moved into LDS
// nor read; every piece keeps its place in the row image and in the row buffers (the holes are simply not filled).
__device__ __host__ constexpr bool valu_odd_cart(int pool) { return pool == LF_POOL_F16X3; }
constexpr int kOddCartSums = 7;   // m | per harmonic: sin_o (operand U), -cos_o (operand V)
constexpr int kPolarSlots = 10;   // folded mixed tiles: slots below it hold polar kernels, the others cartesian ones

// 5-tap sigma=0.7 kernel, patch_gradients.glsl:22-28
constexpr float kB0 = 0.0096f, kB1 = 0.2054f, kB2 = 0.5699f;

// LDS map of the pooling kernel (bytes)
__device__ __host__ constexpr int row_bytes(bool fold) { return lut_pieces(fold) * 1024; }   // one LUT row image: 24576 (30720)
__device__ __host__ constexpr int ring_off(bool fold) { return 2 * row_bytes(fold); }         // raw patch rows: [wave 8][slot 6][2 KiB]
constexpr int kRowBytes = row_bytes(true), kRingOff = ring_off(true);                         // the folded forms'
constexpr int kRingSlots = 6;
// total: ring_off + waves * kRingSlots * 2048 = 147456 B for 8 waves, 98304 B for 4
// Keypoint mode (SRC = kSrcKeypoints): the ring of a describe wave is filled by a producer wave of the same workgroup, four
// patch rows at a time (a group), so it holds 12 rows: the 8 a describe wave reads while a group is being written + that
// group.  Raw row r of the workgroup's it-th batch lives in slot (8 it + r) mod 12 (32 mod 12 = 8: the numbering simply
// runs on across batches).  4 describe waves: kRingOff + 4 * 12 * 2048 = 147456 B, plus the level table.
// SRC = kSrcKeypointsSplit (round 6; requests of at most 4096 keypoints): the 32 rows of a batch's patches are divided among
// R = 2 or 4 WORKGROUPS (row-split form, see mkd_pool) whose partial pooled sums meet in global memory.
[[maybe_unused]] constexpr int kSrcPatches = 0, kSrcKeypoints = 1, kSrcKeypointsSplit = 2;
constexpr int kRingSlotsKp = 12;
constexpr int kLevelTableBytes = 5 * kMaxPyrLevels * 4;

__device__ __forceinline__ float lane_fetch(int byte_addr, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}

__device__ __forceinline__ void lds_dma16(const void *gsrc, void *ldst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)ldst, 16, 0, 0);
}
// (uniform base) + (32-bit lane offset).  The base goes through an opaque SGPR constraint so that hipcc cannot
// re-associate it with the lane offset into a per-lane 64-bit base plus a uniform offset (which it then hoists).
// LIVE = false (LF_ABLATE_ROW_DMA, a timing-only build): the addresses are formed and the request is left out.
template <bool LIVE = true>
__device__ __forceinline__ void lds_dma16_sv(const unsigned char *uniform_base, unsigned lane_off, void *ldst) {
    asm("" : "+s"(uniform_base));
    // volatile: keeps the 32-bit offset's zero-extension in the basic block of its use, where instruction selection can
    // fold it into the addressing mode (hoisted out of the row loop it becomes a 64-bit VGPR pair and an add per request)
    asm volatile("" : "+v"(lane_off));
    if constexpr (LIVE) lds_dma16(uniform_base + lane_off, ldst);
    else asm volatile("" ::"s"(uniform_base), "v"(lane_off), "s"((unsigned)(size_t)(__attribute__((address_space(3))) void *)ldst) : "memory");
}

// Global addresses of the DMA requests are formed as (wave-uniform 64-bit base) + (32-bit lane offset), in that order:
// hipcc then selects the SGPR-base form `global_load_lds_dwordx4 v_off, s[base:base+1]`, which costs no 64-bit VALU add and
// no VGPR pair per request (written as per-lane pointer + uniform offset, every request carried its own v_lshl_add_u64
// and the hoisted address pairs were spilled).
// one LUT row (24 pieces; 30 unfolded) into an LDS row buffer, piece p by wave p mod W (the first waves take one piece more).
// ODDV (valu_odd_cart): the two pieces of tile 2 of each group stay behind -- 16 pieces, the i-th of them piece i + 2 (i / 4).
template <int W, bool FOLD, bool ODDV, bool LIVE = true>
__device__ __forceinline__ void issue_lut_row(const unsigned char *__restrict__ lut_rows, int row,
                                              unsigned char *lds_row, int wave, int lane) {
    static_assert(!ODDV || FOLD, "the folded forms' tiles");
    constexpr int kPieces = ODDV ? lut_pieces(FOLD) - 8 : lut_pieces(FOLD);
    const unsigned lane16 = (unsigned)lane * 16u;
#pragma unroll
    for (int j = 0; j < (kPieces + W - 1) / W; ++j) {
        // uniform; `wave` is in [0, W), so where W divides the pieces every wave takes every turn and nothing is asked (asked,
        // the two answers of f16x3's 8-wave form sit in registers through the row loop, which has none to spare)
        if (kPieces % W == 0 || wave + W * j < kPieces) {
            const int i = wave + W * j, piece = ODDV ? i + 2 * (i >> 2) : i;
            const unsigned char *g = lut_rows + ((size_t)row * row_bytes(FOLD) + (size_t)piece * 1024);   // uniform
            lds_dma16_sv<LIVE>(g, lane16, lds_row + piece * 1024);
        }
    }
}

// Whitening fragments are staged through the two LUT row buffers (idle during the epilogue) one 16 KiB step at a
// time, shared by the workgroup's waves: three slots, placed so that step 0 lies in row buffer 0 (it is requested during
// patch row 31, when only that buffer is free) and the last step in row buffer 1 (so that LUT row 0 of the next batch
// can be requested into buffer 0 while the last step is still being consumed).
constexpr int kWStepBytes = 16384;
__device__ __forceinline__ constexpr int wstage_slot(int step) { return step % 3 == 0 ? 0 : (step % 3 == 1 ? 32768 : 16384); }
static_assert(wstage_slot(0) + kWStepBytes <= row_bytes(true) && wstage_slot(10) >= row_bytes(false) &&
              wstage_slot(10) + kWStepBytes <= 2 * row_bytes(true), "both forms' row buffers");

template <int W>
__device__ __forceinline__ void issue_w_step(const unsigned char *__restrict__ wfrag, int step, unsigned char *lds,
                                             int wave, int lane) {
    const unsigned lane16 = (unsigned)lane * 16u;
    unsigned char *d = lds + wstage_slot(step);
#pragma unroll
    for (int j = 0; j < 16 / W; ++j) {
        const unsigned char *g = wfrag + ((size_t)step * kWStepBytes + (size_t)(wave + W * j) * 1024);   // uniform
        lds_dma16_sv(g, lane16, d + (wave + W * j) * 1024);
    }
}

// One ticket of a launch's claim counter into lane 0's `t` (mkd_pool, claim forms): a relaxed agent-scope fetch-and-add
// of 1, REQUESTED only -- `t` holds the ticket once the caller has waited for vmcnt(0) with `t` as an operand of the wait.
// Written out: the builtin goes through hipcc's wave-level aggregation of atomics, which waits for the result on the spot.
__device__ __forceinline__ void request_ticket(unsigned *counter, unsigned &t) {
    unsigned long long exec_was;
    asm volatile("s_mov_b64 %1, exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "global_atomic_add %0, %2, %3, %4 sc0\n\t"
                 "s_mov_b64 exec, %1"
                 : "+v"(t), "=&s"(exec_was)
                 : "v"(0u), "v"(1u), "s"(counter)
                 : "memory");
}
__device__ __forceinline__ void await_ticket(unsigned &t) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(t)::"memory"); }

// Counted wait on the vector-memory counter.  INVARIANT: between the DMA requests this counts and the wait itself, the
// wave must issue no other vector-memory instruction -- in particular no scratch spill: spill stores share vmcnt and retire
// out of order with respect to loads, so one in flight lets the wait pass before the counted DMA has landed.  hipcc
// inserts spills on its own when registers run out; the Makefile therefore rejects an f16 build of this kernel whose
// ScratchSize is not 0 (tools/check_scratch.py), and the raw_out verification tap, which stores, waits with vmcnt(0).
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// one raw patch row, `row` in [0, 31] (16 patches x 128 B), of this wave into ring slot `slot`.  The one-row patch forms keep
// copies of rows 0 and 31 in slots of their own for the rows beyond the patch (clamp_row); the pair forms request no row twice.
// src = the wave's (uniform) first patch, lane_off = byte offset of the lane's patch and 16-byte chunk from it.
struct RawSrc { const unsigned char *base; unsigned lane_off; };
__device__ __forceinline__ constexpr int clamp_row(int row) { return row < 0 ? 0 : (row > 31 ? 31 : row); }
template <bool LIVE = true>
__device__ __forceinline__ void issue_raw_row(const RawSrc &src, int row, unsigned char *ring, int slot) {
    const unsigned char *g = src.base + row * 128;   // uniform
    lds_dma16_sv<LIVE>(g, src.lane_off, ring + slot * 2048);
    lds_dma16_sv<LIVE>(g + 64, src.lane_off, ring + slot * 2048 + 1024);
}

// No implicit contraction in the describe kernel (down to the end of mkd_pool): every fused multiply-add in it is written
// as one.  The 4-wave and 8-wave forms are separate instantiations, and left to itself hipcc may contract an
// expression in one and not in the other -- a descriptor must not depend on the size of the request it was part of
// (tests/test_gpu_parity.py::test_full_size_properties compares the two forms bit for bit).
#pragma clang fp contract(off)

// max(a, b, 1e-30) in one instruction (a, b >= 0): the larger gradient component as a divisor that is never 0
__device__ __forceinline__ float max3_tiny(float a, float b) {
    return __builtin_fmaxf(__builtin_fmaxf(a, b), 1e-30f);   // v_max3_f32, with the |.| of its operands folded in
}

// cos/sin of the gradient angle theta = -atan2(gy over gx), for a pair of pixels.
template <int ANGLE>
__device__ __forceinline__ void gradient_direction(f32x2 gx, f32x2 gy, f32x2 r2, f32x2 &ct, f32x2 &st) {
    if (ANGLE == LF_ANGLE_EXACT || ANGLE == LF_ANGLE_EXACT_ZERO) {
        // r2 = gx^2 + gy^2 comes from the caller (it is the magnitude's radicand before its epsilon)
        const f32x2 inv = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
        const f32x2 c = gx * inv, s = -gy * inv;
        // EXACT: angle 0 only for the null gradient (the CPU twin's atan2(0, 0)); EXACT_ZERO: wherever gx == 0, which is
        // the shader's convention (atan2.glsl:33-38) -- the one place where the two angle definitions are far apart
        const bool z0 = ANGLE == LF_ANGLE_EXACT ? r2.x == 0.f : gx.x == 0.f;
        const bool z1 = ANGLE == LF_ANGLE_EXACT ? r2.y == 0.f : gx.y == 0.f;
        ct = f32x2{z0 ? 1.f : c.x, z1 ? 1.f : c.y};
        st = f32x2{z0 ? 0.f : s.x, z1 ? 0.f : s.y};
    } else {
        // atan2.glsl:19-46 called as atan2(x = gx, y = gy): a = (smaller / larger component), p = poly(a), then
        //   swap (|x| < |y|):  res = sign(a) pi/2 - p;   x < 0: res += +-pi.
        // poly is odd, so with a' = |a| and p' = poly(a') = |p| these branches are the octant symmetries
        //   (|cos res|, |sin res|) = swap ? (sin p', cos p') : (cos p', sin p'),  sign(cos res) = sign(x),  sign(sin res) = sign(y)
        // (case by case from the three lines above), and the first octant needs no signs and no select of num / den:
        const float ax0 = fabsf(gx.x), ay0 = fabsf(gy.x), ax1 = fabsf(gx.y), ay1 = fabsf(gy.y);
        // gx == 0: the shader returns angle 0 both for atan2(0, 0) and (its quirk) for atan2(0, y != 0), i.e.
        // (cos, sin) = (1, 0).  That is the un-swapped branch at a = 0 (p = 0: cos p = 1, sin p = 0), so such a pixel simply
        // does not swap, and the denominator is kept away from 0 (0 x rcp(0) would be NaN) -- no selects afterwards
        const bool sw0 = ax0 < ay0 && gx.x != 0.f, sw1 = ax1 < ay1 && gx.y != 0.f;
        const f32x2 mn = {__builtin_fminf(ax0, ay0), __builtin_fminf(ax1, ay1)};
        const f32x2 mx = {max3_tiny(ax0, ay0), max3_tiny(ax1, ay1)};
        const f32x2 a = mn * f32x2{__builtin_amdgcn_rcpf(mx.x), __builtin_amdgcn_rcpf(mx.y)};
        const f32x2 s = a * a;
        f32x2 p = pk_fma(s, pk_set(-0.0117212f), pk_set(0.05265332f));
        p = pk_fma(s, p, pk_set(-0.11643287f));
        p = pk_fma(s, p, pk_set(0.19354346f));
        p = pk_fma(s, p, pk_set(-0.33262347f));
        p = pk_fma(s, p, pk_set(0.99997726f));
        p = a * p;
        // 0 <= p <= 0.7854: minimax fits in p^2 (Remez on [0, (pi/4)^2], float64, rounded to f32) -- 2.4e-9 / 2.8e-8
        // before rounding, one term shorter than the Taylor series of the same accuracy
        const f32x2 p2 = p * p;
        f32x2 sn = pk_fma(p2, pk_set(-0.000195038549f), pk_set(0.0083320355f));
        sn = pk_fma(p2, sn, pk_set(-0.166666508f));
        sn = pk_fma(p2, sn, pk_set(1.f));
        sn = p * sn;
        f32x2 cs = pk_fma(p2, pk_set(-0.00135857589f), pk_set(0.0416550152f));
        cs = pk_fma(p2, cs, pk_set(-0.499998569f));
        cs = pk_fma(p2, cs, pk_set(1.f));
        // cos theta = cos res: sign of gx; sin theta = -sin res: opposite sign of gy (sn, cs >= 0: OR the sign bit in)
        const unsigned sgn = 0x80000000u;
        float cr0 = __uint_as_float(__float_as_uint(sw0 ? sn.x : cs.x) | (__float_as_uint(gx.x) & sgn));
        float cr1 = __uint_as_float(__float_as_uint(sw1 ? sn.y : cs.y) | (__float_as_uint(gx.y) & sgn));
        float sr0 = __uint_as_float(__float_as_uint(sw0 ? cs.x : sn.x) | (~__float_as_uint(gy.x) & sgn));
        float sr1 = __uint_as_float(__float_as_uint(sw1 ? cs.y : sn.y) | (~__float_as_uint(gy.y) & sgn));
        ct = f32x2{cr0, cr1};
        st = f32x2{sr0, sr1};
    }
}

// The same for the lane's four pixel pairs at once, written step by step across the pairs: the polynomial chains of a
// pair are serial (each packed fma waits for the one before it, and hipcc pads back-to-back dependent packed operations
// with s_nop), the four pairs are independent -- in this order every instruction has three others between it and the one
// it depends on.  Same operations on the same values as gradient_direction: bit-identical.
template <int ANGLE>
__device__ __forceinline__ void gradient_direction4(const f32x2 (&gx)[4], const f32x2 (&gy)[4], const f32x2 (&r2)[4],
                                                    f32x2 (&ct)[4], f32x2 (&st)[4]) {
    if (ANGLE != LF_ANGLE_SHADER) {
#pragma unroll
        for (int e = 0; e < 4; ++e) gradient_direction<ANGLE>(gx[e], gy[e], r2[e], ct[e], st[e]);
        return;
    }
    f32x2 a[4], s[4], p[4], p2[4], sn[4], cs[4];
    bool sw0[4], sw1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ax0 = fabsf(gx[e].x), ay0 = fabsf(gy[e].x), ax1 = fabsf(gx[e].y), ay1 = fabsf(gy[e].y);
        sw0[e] = ax0 < ay0 && gx[e].x != 0.f;   // gx == 0 -> (1, 0): the un-swapped branch at a = 0 (see gradient_direction)
        sw1[e] = ax1 < ay1 && gx[e].y != 0.f;
        const f32x2 mn = {__builtin_fminf(ax0, ay0), __builtin_fminf(ax1, ay1)};
        const f32x2 mx = {max3_tiny(ax0, ay0), max3_tiny(ax1, ay1)};
        a[e] = mn * f32x2{__builtin_amdgcn_rcpf(mx.x), __builtin_amdgcn_rcpf(mx.y)};
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = a[e] * a[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = pk_fma(s[e], pk_set(-0.0117212f), pk_set(0.05265332f));
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = pk_fma(s[e], p[e], pk_set(-0.11643287f));
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = pk_fma(s[e], p[e], pk_set(0.19354346f));
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = pk_fma(s[e], p[e], pk_set(-0.33262347f));
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = pk_fma(s[e], p[e], pk_set(0.99997726f));
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = a[e] * p[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) p2[e] = p[e] * p[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sn[e] = pk_fma(p2[e], pk_set(-0.000195038549f), pk_set(0.0083320355f));
        cs[e] = pk_fma(p2[e], pk_set(-0.00135857589f), pk_set(0.0416550152f));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sn[e] = pk_fma(p2[e], sn[e], pk_set(-0.166666508f));
        cs[e] = pk_fma(p2[e], cs[e], pk_set(-0.499998569f));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sn[e] = pk_fma(p2[e], sn[e], pk_set(1.f));
        cs[e] = pk_fma(p2[e], cs[e], pk_set(1.f));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sn[e] = p[e] * sn[e];
    const unsigned sgn = 0x80000000u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float cr0 = __uint_as_float(__float_as_uint(sw0[e] ? sn[e].x : cs[e].x) | (__float_as_uint(gx[e].x) & sgn));
        float cr1 = __uint_as_float(__float_as_uint(sw1[e] ? sn[e].y : cs[e].y) | (__float_as_uint(gx[e].y) & sgn));
        float sr0 = __uint_as_float(__float_as_uint(sw0[e] ? cs[e].x : sn[e].x) | (~__float_as_uint(gy[e].x) & sgn));
        float sr1 = __uint_as_float(__float_as_uint(sw1[e] ? cs[e].y : sn[e].y) | (~__float_as_uint(gy[e].y) & sgn));
        ct[e] = f32x2{cr0, cr1};
        st[e] = f32x2{sr0, sr1};
    }
}

// ---- B fragments (LUT) and A fragments (streams) -------------------------------------------------
// One unique LUT tile = two 1 KiB pieces: f32: pixels 0-3 / 4-7 of the lane's segment (K = 4 MFMAs);
// f16: hi / lo halves of all 8 pixels (K = 32 MFMAs).  16 B per lane either way.
struct BFrag { u32x4 p0, p1; };

__device__ __forceinline__ BFrag load_b(const unsigned char *brow, int ut) {   // ut: a constant after unrolling
    BFrag b;
    if constexpr (ablate::kNoFragmentReads) {
        b.p0 = u32x4{(unsigned)ut, 1u, 2u, 3u};
        b.p1 = b.p0;
        return b;
    }
    b.p0 = *reinterpret_cast<const u32x4 *>(brow + (ut * 2 + 0) * 1024);
    b.p1 = *reinterpret_cast<const u32x4 *>(brow + (ut * 2 + 1) * 1024);
    return b;
}

__device__ __forceinline__ unsigned pack_rtz(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
}

// A operand of one stream: f32: the 8 values themselves; f16: hi = f16 truncation, lo = f16(a - hi)
template <int POOL> struct AFrag;
template <> struct AFrag<LF_POOL_F32> {
    float v[8];
    __device__ __forceinline__ void set(const f32x2 (&a)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[2 * e] = a[e].x; v[2 * e + 1] = a[e].y; }
    }
};
template <> struct AFrag<LF_POOL_F16X3> {
    u32x4 hi, lo;
    __device__ __forceinline__ void set(const f32x2 (&a)[4]) {
        // residual a - hi as ONE v_fma_mix_f32 (f32 x f32 - f16); the factor 1 is hidden from hipcc, which otherwise
        // folds the fma into an unpack plus a subtract
        if constexpr (ablate::kNoSplit) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { hi[e] = __float_as_uint(a[e].x); lo[e] = __float_as_uint(a[e].y); }
            return;
        }
        // (written step by step across the four pairs: conversion, residuals, conversion are each one dependent on the
        // other; across the pairs they are not)
        float one = 1.f;
        asm("" : "+v"(one));
        float r0[4], r1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) hi[e] = pack_rtz(a[e].x, a[e].y);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float h0 = (float)__builtin_bit_cast(_Float16, (unsigned short)(hi[e] & 0xffffu));
            const float h1 = (float)__builtin_bit_cast(_Float16, (unsigned short)(hi[e] >> 16));
            r0[e] = __builtin_fmaf(a[e].x, one, -h0);
            r1[e] = __builtin_fmaf(a[e].y, one, -h1);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) lo[e] = pack_rtz(r0[e], r1[e]);
    }
    // two streams at once (the cos and sin streams of a harmonic): twice as many independent operations per step
    __device__ __forceinline__ static void set2(AFrag &x, const f32x2 (&a)[4], AFrag &y, const f32x2 (&b)[4]) {
        if constexpr (ablate::kNoSplit) {
            x.set(a);
            y.set(b);
            return;
        }
        float one = 1.f;
        asm("" : "+v"(one));
        float ra0[4], ra1[4], rb0[4], rb1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { x.hi[e] = pack_rtz(a[e].x, a[e].y); y.hi[e] = pack_rtz(b[e].x, b[e].y); }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ra0[e] = __builtin_fmaf(a[e].x, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(x.hi[e] & 0xffffu)));
            ra1[e] = __builtin_fmaf(a[e].y, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(x.hi[e] >> 16)));
            rb0[e] = __builtin_fmaf(b[e].x, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(y.hi[e] & 0xffffu)));
            rb1[e] = __builtin_fmaf(b[e].y, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(y.hi[e] >> 16)));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { x.lo[e] = pack_rtz(ra0[e], ra1[e]); y.lo[e] = pack_rtz(rb0[e], rb1[e]); }
    }
};

// acc += LUT^T x stream for one (stream, tile): the LUT fragment is the MFMA's A operand (rows = packed
// columns), the stream its B operand (columns = patches), so a lane ends up holding packed columns
// 16t + 4(lane >> 4) + i of ITS OWN patch (lane & 15) -- which is what the fused epilogue needs.
// `part` selects one third of the f16 split so callers can interleave independent accumulators between the
// dependent MFMAs of one tile.
template <int POOL, int PART>
__device__ __forceinline__ void mma_part(const AFrag<POOL> &a, const BFrag &b, f32x4 &acc) {
    static_assert(POOL == LF_POOL_F32 || POOL == LF_POOL_F16X3, "the three-term / f32 forms");
    if constexpr (ablate::kNoMma && POOL == LF_POOL_F16X3) {   // (operands kept alive)
        asm volatile("" ::"v"(a.hi), "v"(a.lo), "v"(b.p0), "v"(b.p1));
        return;
    }
    if constexpr (POOL == LF_POOL_F32) {
        const f32x4 b0 = __builtin_bit_cast(f32x4, b.p0), b1 = __builtin_bit_cast(f32x4, b.p1);
        if (PART == 0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b0[e], a.v[e], acc, 0, 0, 0);
        } else if (PART == 1) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b0[3], a.v[3], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b1[0], a.v[4], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b1[1], a.v[5], acc, 0, 0, 0);
        } else {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b1[2], a.v[6], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b1[3], a.v[7], acc, 0, 0, 0);
        }
    } else {
        const f16x8 bh = __builtin_bit_cast(f16x8, b.p0), bl = __builtin_bit_cast(f16x8, b.p1);
        const f16x8 ah = __builtin_bit_cast(f16x8, a.hi), al = __builtin_bit_cast(f16x8, a.lo);
        if (PART == 0) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, al, acc, 0, 0, 0);
        else if (PART == 1) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, ah, acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, ah, acc, 0, 0, 0);
    }
}

// Blurred row of this lane's segment from the raw-row ring (patch_gradients.glsl:72-92): vertical 5 taps over five ring
// slots, then horizontal 5 taps with the neighbours fetched from lanes -/+16.  The two halves are separate functions: patch
// mode runs the vertical half for two rows at once (vblur_pair).
// Vertical half.  The lane's two 16-byte blocks of a raw row sit at ring_a and ring_b + slot * 2048; slot_of_tap(i) = ring slot of
// the i-th of the five raw rows.  v = the eight pixels, first block then second, both in ascending x.
template <class SlotOfTap>
__device__ __forceinline__ void vblur_row(const unsigned char *ring_a, const unsigned char *ring_b, SlotOfTap slot_of_tap,
                                          float (&v)[8]) {
    if constexpr (ablate::kNoFrontEnd) {   // no blur: the first tap's raw row as it is
        const int sl = slot_of_tap(0);
        const f32x4 a_ = *reinterpret_cast<const f32x4 *>(ring_a + sl * 2048);
        const f32x4 b_ = *reinterpret_cast<const f32x4 *>(ring_b + sl * 2048);
#pragma unroll
        for (int x = 0; x < 4; ++x) { v[x] = a_[x]; v[4 + x] = b_[x]; }
        return;
    }
    const float kk[5] = {kB0, kB1, kB2, kB1, kB0};
    f32x2 v2[4];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int sl = slot_of_tap(i);
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(ring_a + sl * 2048);
        const f32x4 hi = *reinterpret_cast<const f32x4 *>(ring_b + sl * 2048);
        const f32x2 r[4] = {{lo[0], lo[1]}, {lo[2], lo[3]}, {hi[0], hi[1]}, {hi[2], hi[3]}};
#pragma unroll
        for (int e = 0; e < 4; ++e) v2[e] = i == 0 ? pk_set(kk[0]) * r[e] : pk_fma(pk_set(kk[i]), r[e], v2[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = v2[e].x; v[2 * e + 1] = v2[e].y; }
}

// Vertical half of TWO blurred rows at once (patch mode's row pairs): the NR raw rows the two need between them are read
// from the ring once each -- row j from slot_of_row(j) -- and feed two accumulations, tap i of the first row being raw row
// tap_a(i) and of the second tap_b(i).  Each accumulation is vblur_row's: the same five operations in the same order, a
// replicated row (the patch's first and last rows) as a tap of its own with its own coefficient.
template <int NR, class SlotOfRow, class TapA, class TapB>
__device__ __forceinline__ void vblur_pair(const unsigned char *ring_a, const unsigned char *ring_b, SlotOfRow slot_of_row,
                                           TapA tap_a, TapB tap_b, float (&va)[8], float (&vb)[8]) {
    f32x2 r[NR][4];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int sl = slot_of_row(j);
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(ring_a + sl * 2048);
        const f32x4 hi = *reinterpret_cast<const f32x4 *>(ring_b + sl * 2048);
        r[j][0] = f32x2{lo[0], lo[1]}; r[j][1] = f32x2{lo[2], lo[3]};
        r[j][2] = f32x2{hi[0], hi[1]}; r[j][3] = f32x2{hi[2], hi[3]};
    }
    f32x2 a2[4], b2[4];
    if constexpr (ablate::kNoFrontEnd) {   // no blur: the first taps' raw rows as they are
#pragma unroll
        for (int e = 0; e < 4; ++e) { a2[e] = r[tap_a(0)][e]; b2[e] = r[tap_b(0)][e]; }
    } else {
        const float kk[5] = {kB0, kB1, kB2, kB1, kB0};
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int ja = tap_a(i), jb = tap_b(i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a2[e] = i == 0 ? pk_set(kk[0]) * r[ja][e] : pk_fma(pk_set(kk[i]), r[ja][e], a2[e]);
                b2[e] = i == 0 ? pk_set(kk[0]) * r[jb][e] : pk_fma(pk_set(kk[i]), r[jb][e], b2[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        va[2 * e] = a2[e].x; va[2 * e + 1] = a2[e].y;
        vb[2 * e] = b2[e].x; vb[2 * e + 1] = b2[e].y;
    }
}

// Horizontal half: vb = the lane's eight pixels of the vertically blurred row.  Returns the row plus its x-1 / x+8 neighbours.
__device__ __forceinline__ void hblur_row(const float (&vb)[8], int addr_l, int addr_r, bool has_l, bool has_r, float (&out)[8],
                                          float &out_l, float &out_r) {
    if constexpr (ablate::kNoFrontEnd) {
#pragma unroll
        for (int x = 0; x < 8; ++x) out[x] = vb[x];
        out_l = out[0];
        out_r = out[7];
        return;
    }
    float ext[12];
    const float l0 = lane_fetch(addr_l, vb[6]), l1 = lane_fetch(addr_l, vb[7]);
    const float r0 = lane_fetch(addr_r, vb[0]), r1 = lane_fetch(addr_r, vb[1]);
    ext[0] = has_l ? l0 : vb[0];
    ext[1] = has_l ? l1 : vb[0];
    ext[10] = has_r ? r0 : vb[7];
    ext[11] = has_r ? r1 : vb[7];
#pragma unroll
    for (int x = 0; x < 8; ++x) ext[2 + x] = vb[x];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        // (the first tap as an fma onto +0.0: the same bits as the product for every non-zero result, and +0.0 where the
        //  factor is -0.0.  A product of a negative denormal that underflows still rounds to -0.0 -- the caller normalises
        //  gx itself, see "left - right" in the row loop)
        float s = ablate::kMulFirstTap ? kB0 * ext[x] : fmaf(kB0, ext[x], 0.0f);
        s = fmaf(kB1, ext[x + 1], s);
        s = fmaf(kB2, ext[x + 2], s);
        s = fmaf(kB1, ext[x + 3], s);
        s = fmaf(kB0, ext[x + 4], s);
        out[x] = s;
    }
    const float hl = lane_fetch(addr_l, out[7]), hr = lane_fetch(addr_r, out[0]);
    out_l = has_l ? hl : out[0];
    out_r = has_r ? hr : out[7];
}

template <class SlotOfTap>
__device__ __forceinline__ void blur_row_impl(const unsigned char *ring_lane, SlotOfTap slot_of_tap, int addr_l, int addr_r,
                                              bool has_l, bool has_r, float (&out)[8], float &out_l, float &out_r) {
    float vb[8];
    vblur_row(ring_lane, ring_lane + 256, slot_of_tap, vb);
    hblur_row(vb, addr_l, addr_r, has_l, has_r, out, out_l, out_r);
}

// The same for the folded forms' lane map.  The lane's two blocks of the raw row come from ring_a (x in [4q, 4q+4)) and
// ring_b (x in [28-4q, 32-4q)).  out[0..3] = the first block in ascending x, out[4..7] = the second in DESCENDING x: out[4 + i]
// is the mirror pixel of out[i].  Each block needs two neighbours a side of the vertically blurred row and one of the
// blurred row: the first block's from the first blocks of lanes -/+16, the second block's from the second blocks of
// lanes +/-16; where the two blocks touch (q == 3) they are the lane's own values, at the patch's edges (q == 0) they replicate.
// nb = the blurred row at x = 4q-1, 4q+4, 27-4q, 32-4q.  Per pixel the arithmetic and its order are blur_row_impl's.
__device__ __forceinline__ void hblur_row_fold(const float (&v)[8], int addr_l, int addr_r, bool has_l, bool has_r,
                                               float (&out)[8], float (&nb)[4]) {
    if constexpr (ablate::kNoFrontEnd) {
#pragma unroll
        for (int x = 0; x < 4; ++x) { out[x] = v[x]; out[4 + x] = v[7 - x]; }
        nb[0] = out[0]; nb[1] = out[3]; nb[2] = out[7]; nb[3] = out[4];
        return;
    }
    // vertically blurred (vblur_row), both blocks in ascending x
    const float va[4] = {v[0], v[1], v[2], v[3]}, vb[4] = {v[4], v[5], v[6], v[7]};
    float ea[8], eb[8];
    {
        const float la0 = lane_fetch(addr_l, va[2]), la1 = lane_fetch(addr_l, va[3]);   // x = 4q-2, 4q-1
        const float rb0 = lane_fetch(addr_l, vb[0]), rb1 = lane_fetch(addr_l, vb[1]);   // x = 32-4q, 33-4q
        const float ra0 = lane_fetch(addr_r, va[0]), ra1 = lane_fetch(addr_r, va[1]);   // x = 4q+4, 4q+5
        const float lb0 = lane_fetch(addr_r, vb[2]), lb1 = lane_fetch(addr_r, vb[3]);   // x = 26-4q, 27-4q
        ea[0] = has_l ? la0 : va[0];
        ea[1] = has_l ? la1 : va[0];
        ea[6] = has_r ? ra0 : vb[0];
        ea[7] = has_r ? ra1 : vb[1];
        eb[0] = has_r ? lb0 : va[2];
        eb[1] = has_r ? lb1 : va[3];
        eb[6] = has_l ? rb0 : vb[3];
        eb[7] = has_l ? rb1 : vb[3];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) { ea[2 + x] = va[x]; eb[2 + x] = vb[x]; }
    float ob[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {   // (the first tap as an fma onto +0.0: see blur_row_impl)
        float s = ablate::kMulFirstTap ? kB0 * ea[x] : fmaf(kB0, ea[x], 0.0f);
        s = fmaf(kB1, ea[x + 1], s);
        s = fmaf(kB2, ea[x + 2], s);
        s = fmaf(kB1, ea[x + 3], s);
        s = fmaf(kB0, ea[x + 4], s);
        out[x] = s;
        float t = ablate::kMulFirstTap ? kB0 * eb[x] : fmaf(kB0, eb[x], 0.0f);
        t = fmaf(kB1, eb[x + 1], t);
        t = fmaf(kB2, eb[x + 2], t);
        t = fmaf(kB1, eb[x + 3], t);
        t = fmaf(kB0, eb[x + 4], t);
        ob[x] = t;
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) out[4 + x] = ob[3 - x];
    const float hal = lane_fetch(addr_l, out[3]), hbr = lane_fetch(addr_l, ob[0]);
    const float har = lane_fetch(addr_r, out[0]), hbl = lane_fetch(addr_r, ob[3]);
    nb[0] = has_l ? hal : out[0];
    nb[1] = has_r ? har : ob[0];
    nb[2] = has_r ? hbl : out[3];
    nb[3] = has_l ? hbr : ob[3];
}

// The pair forms' horizontal half (patch mode, f16x3): hblur_row_fold with the twelve lane fetches replaced by RECORDS in an
// LDS area private to the wave (2 KiB: two lane-linear planes of 16 bytes a lane, plane 0 = v[0..3], plane 1 = v[4..7],
// 1 KiB apart).  A lane writes its eight vertical sums (2 ds_write_b128) and reads, from the record of lane - 16, v[2..5]
// and, from that of lane + 16, v[0], v[1], v[6], v[7]: one ds_read2_b64 each.  The blurred row's four edge pixels go the
// same way through plane 0, as {out[3], ob[0], out[0], ob[3]}: one write and two 8-byte reads, which hipcc issues as one
// ds_read2_b64.  6 LDS instructions instead of 12.  halo_records is the first exchange, hblur_row_fold_rec the filter and the second.
// rec = the lane's record LESS kRecBack bytes, so that the record of lane - 16 lies at rec + 0, the lane's own at
// rec + 256 and that of lane + 16 at rec + 512: one address register, every distance an instruction offset.  A lane without a
// neighbour (q == 0 on the left, q == 3 on the right) reads the 256 bytes of the wave's LDS next to the area on that side
// and drops them in the has_l / has_r selects, as the fetches' wrapped lanes were dropped.
// Order: the exchange is inside ONE wave, whose LDS instructions execute in the order of issue for all 64 lanes -- no
// barrier; the empty asm statements keep hipcc from moving a read above the write it depends on (to the compiler a lane
// reads what it never wrote), and the area may be written again as soon as the earlier reads have been issued.
// The values, the selects and the arithmetic are hblur_row_fold's: the descriptors keep their bits.
constexpr int kRecBack = 256, kRecPlane = 1024;
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) f32x2 lds_f32x2;
// the four pairs a lane takes from its neighbours' records of the vertical sums
struct Halo { f32x2 la, rb, ra, lb; };
__device__ __forceinline__ Halo halo_records(const float (&v)[8], lds_u8 *rec) {
    Halo h{pk_set(0.f), pk_set(0.f), pk_set(0.f), pk_set(0.f)};
    if constexpr (ablate::kNoFrontEnd) return h;
    lds_u8 *own = rec + kRecBack;
    const lds_u8 *left = rec, *right = rec + 2 * kRecBack;
    *reinterpret_cast<lds_f32x4 *>(own) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<lds_f32x4 *>(own + kRecPlane) = f32x4{v[4], v[5], v[6], v[7]};
    asm volatile("" ::: "memory");
    h.la = *reinterpret_cast<const lds_f32x2 *>(left + 8);                // va[2], va[3] of lane - 16: x = 4q-2, 4q-1
    h.rb = *reinterpret_cast<const lds_f32x2 *>(left + kRecPlane);        // vb[0], vb[1] of lane - 16: x = 32-4q, 33-4q
    h.ra = *reinterpret_cast<const lds_f32x2 *>(right);                   // va[0], va[1] of lane + 16: x = 4q+4, 4q+5
    h.lb = *reinterpret_cast<const lds_f32x2 *>(right + kRecPlane + 8);   // vb[2], vb[3] of lane + 16: x = 26-4q, 27-4q
    asm volatile("" ::: "memory");
    return h;
}
__device__ __forceinline__ void hblur_row_fold_rec(const float (&v)[8], const Halo &h, lds_u8 *rec, bool has_l, bool has_r,
                                                   float (&out)[8], float (&nb)[4]) {
    if constexpr (ablate::kNoFrontEnd) {
#pragma unroll
        for (int x = 0; x < 4; ++x) { out[x] = v[x]; out[4 + x] = v[7 - x]; }
        nb[0] = out[0]; nb[1] = out[3]; nb[2] = out[7]; nb[3] = out[4];
        return;
    }
    const float va[4] = {v[0], v[1], v[2], v[3]}, vb[4] = {v[4], v[5], v[6], v[7]};
    lds_u8 *own = rec + kRecBack;
    const lds_u8 *left = rec, *right = rec + 2 * kRecBack;
    const f32x2 la = h.la, rb = h.rb, ra = h.ra, lb = h.lb;
    float ea[8], eb[8];
    ea[0] = has_l ? la.x : va[0];
    ea[1] = has_l ? la.y : va[0];
    ea[6] = has_r ? ra.x : vb[0];
    ea[7] = has_r ? ra.y : vb[1];
    eb[0] = has_r ? lb.x : va[2];
    eb[1] = has_r ? lb.y : va[3];
    eb[6] = has_l ? rb.x : vb[3];
    eb[7] = has_l ? rb.y : vb[3];
#pragma unroll
    for (int x = 0; x < 4; ++x) { ea[2 + x] = va[x]; eb[2 + x] = vb[x]; }
    float ob[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {   // (the first tap as an fma onto +0.0: see blur_row_impl)
        float s = ablate::kMulFirstTap ? kB0 * ea[x] : fmaf(kB0, ea[x], 0.0f);
        s = fmaf(kB1, ea[x + 1], s);
        s = fmaf(kB2, ea[x + 2], s);
        s = fmaf(kB1, ea[x + 3], s);
        s = fmaf(kB0, ea[x + 4], s);
        out[x] = s;
        float t = ablate::kMulFirstTap ? kB0 * eb[x] : fmaf(kB0, eb[x], 0.0f);
        t = fmaf(kB1, eb[x + 1], t);
        t = fmaf(kB2, eb[x + 2], t);
        t = fmaf(kB1, eb[x + 3], t);
        t = fmaf(kB0, eb[x + 4], t);
        ob[x] = t;
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) out[4 + x] = ob[3 - x];
    *reinterpret_cast<lds_f32x4 *>(own) = f32x4{out[3], ob[0], out[0], ob[3]};   // (behind the reads of plane 0 above: issue order)
    asm volatile("" ::: "memory");
    const f32x2 el = *reinterpret_cast<const lds_f32x2 *>(left);        // out[3], ob[0] of lane - 16
    const f32x2 er = *reinterpret_cast<const lds_f32x2 *>(right + 8);   // out[0], ob[3] of lane + 16
    asm volatile("" ::: "memory");
    nb[0] = has_l ? el.x : out[0];
    nb[1] = has_r ? er.x : ob[0];
    nb[2] = has_r ? er.y : out[3];
    nb[3] = has_l ? el.y : ob[3];
}

template <class SlotOfTap>
__device__ __forceinline__ void blur_row_fold_impl(const unsigned char *ring_a, const unsigned char *ring_b, SlotOfTap slot_of_tap,
                                                   int addr_l, int addr_r, bool has_l, bool has_r, float (&out)[8],
                                                   float (&nb)[4]) {
    float v[8];
    vblur_row(ring_a, ring_b, slot_of_tap, v);
    hblur_row_fold(v, addr_l, addr_r, has_l, has_r, out, nb);
}

// Folds a stream about the row's middle: s[0], s[1] = the lane's first block, s[2], s[3] = the mirror pixels of the same.
__device__ __forceinline__ void fold_sum(const f32x2 (&s)[4], f32x2 &e0, f32x2 &e1) { e0 = s[0] + s[2]; e1 = s[1] + s[3]; }
__device__ __forceinline__ void fold_diff(const f32x2 (&s)[4], f32x2 &o0, f32x2 &o1) { o0 = s[0] - s[2]; o1 = s[1] - s[3]; }
__device__ __forceinline__ void fold_diff_rev(const f32x2 (&s)[4], f32x2 &o0, f32x2 &o1) { o0 = s[2] - s[0]; o1 = s[3] - s[1]; }

// The x-odd cartesian kernels' share of one patch row for one stream (valu_odd_cart): h0, h1 = the stream's odd half at
// x = 4q .. 4q+3, fx = the x-profile at the same x, gy = gy_0..2 of the row (wave-uniform).  Six instructions.
__device__ __forceinline__ void odd_cart_row(const f32x2 (&fx)[2], const f32x4 &gy, f32x2 h0, f32x2 h1, float (&oc)[3]) {
    const f32x2 r = pk_fma(fx[1], h1, fx[0] * h0);
    const float t = r.x + r.y;
#pragma unroll
    for (int b = 0; b < 3; ++b) oc[b] = __builtin_fmaf(gy[b], t, oc[b]);
}

// ... and once per batch: accumulator tiles 2 | 3 + 6h + 4 (U), 3 + 6h + 5 (V) from the sums.  Column b of such a tile is c_k
// times the sum over the patch's four lanes; every other column is zero.  As three 16x16x4 f32 matrix instructions per tile
// with A[i][k] = (i == b ? c_k : 0) and B[k][patch] = the sum of lane (patch, q = k): a k-ordered f32 fma chain that lands in the
// packed tiles' own layout (column 4 (lane >> 4) + register of patch lane & 15), with no lane exchange.
__device__ __forceinline__ void rebuild_odd_cart(const float (&oc)[kOddCartSums][3], int lane, f32x4 (&acc)[kAccTiles]) {
    constexpr float kVm[4] = {0.37872374f, 0.51796234f, 0.46882015f, 0.39798096f};   // c_k: kVmN3K8 of mkd_consts.cpp
    // (the twelve selects below are made here, once per batch: as loop invariants of the lane they are hoisted to the top of
    //  the kernel and held in registers through the row loop, which has none to spare)
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int s = 0; s < kOddCartSums; ++s) {
        const int k = (s + 1) / 2, t = s == 0 ? 2 : 3 + 6 * (k - 1) + 4 + ((s - 1) & 1);
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 3; ++b)
            d = __builtin_amdgcn_mfma_f32_16x16x4f32((lane & 15) == b ? kVm[k] : 0.f, oc[s][b], d, 0, 0, 0);
        acc[t] = d;
    }
}

// Harmonics k = 1..3 of the gradient angle (the folded forms).  The recurrence runs on the products themselves,
// (pk, qk) = m (cos, sin)(k theta), as a three-term (Chebyshev) recurrence x_{k+1} = 2 c1 x_k - x_{k-1} with x_0 = (m, 0): one
// instruction per stream and harmonic instead of a rotation of the unit vector (two) plus a product.  After each step the pair is
// folded into the two operands U = [cos_e | sin_o] and V = [sin_e | -cos_o] (mkd_consts.hpp), which meet the SAME three LUT
// tiles: 6 products (18 matrix instructions, f16x3) per harmonic, issued term by term across the six accumulators.  `g` holds
// the fragments of the harmonic's first tile on entry (prefetched by the caller) and the next harmonic's on exit.
// valu_odd_cart(POOL): tile 2 is not met -- 4 products (12 matrix instructions) per harmonic -- and the second halves of U and
// V, sin_o and -cos_o, go through odd_cart_row before the f16 split (fx, gy: see there; oc: the batch's 7 x 3 sums).
template <int POOL>
__device__ __forceinline__ void pool_harmonics(const f32x2 (&m)[4], const f32x2 (&c1)[4], const f32x2 (&s1)[4],
                                               const unsigned char *brow, BFrag &g, f32x4 (&acc)[kAccTiles],
                                               const f32x2 (&fx)[2], const f32x4 &gy, float (&oc)[kOddCartSums][3]) {
    f32x2 pk[4], qk[4], pp[4], qp[4], tc[4];
    AFrag<POOL> au, av;
#pragma unroll
    for (int e = 0; e < 4; ++e) { pk[e] = m[e] * c1[e]; qk[e] = m[e] * s1[e]; tc[e] = c1[e] + c1[e]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        {
            f32x2 u[4], v[4];
            fold_sum(pk, u[0], u[1]);
            fold_diff(qk, u[2], u[3]);
            fold_sum(qk, v[0], v[1]);
            fold_diff_rev(pk, v[2], v[3]);
            if constexpr (valu_odd_cart(POOL)) {
                odd_cart_row(fx, gy, u[2], u[3], oc[1 + 2 * k]);
                odd_cart_row(fx, gy, v[2], v[3], oc[2 + 2 * k]);
            }
            if constexpr (POOL == LF_POOL_F16X3) {
                AFrag<POOL>::set2(au, u, av, v);
            } else {
                au.set(u);
                av.set(v);
            }
        }
        if (k < 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x2 pn = pk_fma(tc[e], pk[e], k == 0 ? -m[e] : -pp[e]);
                const f32x2 qn = k == 0 ? tc[e] * qk[e] : pk_fma(tc[e], qk[e], -qp[e]);
                pp[e] = pk[e]; qp[e] = qk[e];
                pk[e] = pn; qk[e] = qn;
            }
        }
        const int a0 = 3 + 6 * k, u0 = 3 + 3 * k;
        const BFrag t0 = g, t1 = load_b(brow, u0 + 1);
        if constexpr (valu_odd_cart(POOL)) {
            if (k < 2) g = load_b(brow, u0 + 3);
            mma_part<POOL, 0>(au, t0, acc[a0 + 0]); mma_part<POOL, 0>(av, t0, acc[a0 + 1]); mma_part<POOL, 0>(au, t1, acc[a0 + 2]);
            mma_part<POOL, 0>(av, t1, acc[a0 + 3]);
            mma_part<POOL, 1>(au, t0, acc[a0 + 0]); mma_part<POOL, 1>(av, t0, acc[a0 + 1]); mma_part<POOL, 1>(au, t1, acc[a0 + 2]);
            mma_part<POOL, 1>(av, t1, acc[a0 + 3]);
            mma_part<POOL, 2>(au, t0, acc[a0 + 0]); mma_part<POOL, 2>(av, t0, acc[a0 + 1]); mma_part<POOL, 2>(au, t1, acc[a0 + 2]);
            mma_part<POOL, 2>(av, t1, acc[a0 + 3]);
            continue;
        }
        const BFrag t2 = load_b(brow, u0 + 2);
        if (k < 2) g = load_b(brow, u0 + 3);
        mma_part<POOL, 0>(au, t0, acc[a0 + 0]); mma_part<POOL, 0>(av, t0, acc[a0 + 1]); mma_part<POOL, 0>(au, t1, acc[a0 + 2]);
        mma_part<POOL, 0>(av, t1, acc[a0 + 3]); mma_part<POOL, 0>(au, t2, acc[a0 + 4]); mma_part<POOL, 0>(av, t2, acc[a0 + 5]);
        mma_part<POOL, 1>(au, t0, acc[a0 + 0]); mma_part<POOL, 1>(av, t0, acc[a0 + 1]); mma_part<POOL, 1>(au, t1, acc[a0 + 2]);
        mma_part<POOL, 1>(av, t1, acc[a0 + 3]); mma_part<POOL, 1>(au, t2, acc[a0 + 4]); mma_part<POOL, 1>(av, t2, acc[a0 + 5]);
        mma_part<POOL, 2>(au, t0, acc[a0 + 0]); mma_part<POOL, 2>(av, t0, acc[a0 + 1]); mma_part<POOL, 2>(au, t1, acc[a0 + 2]);
        mma_part<POOL, 2>(av, t1, acc[a0 + 3]); mma_part<POOL, 2>(au, t2, acc[a0 + 4]); mma_part<POOL, 2>(av, t2, acc[a0 + 5]);
    }
}

// LF_POOL_F16_FP6 (an experiment kept as a mode; NOTEBOOK.md section 11): the harmonics with hi x hi in f16 (8 instructions per
// harmonic) and BOTH cross terms of every accumulator tile in one v_mfma_scale_f32_16x16x128_f8f6f4 with e2m3 operands (7):
// a lane's 32 K slots hold (a_e, 2048 r_e) of its 8 pixels for the cos stream (fields 0-15 = registers 0-2) and for the
// sin stream (16-31 = registers 3-5), a = the stream value, r = a - f16(a), all divided by the lane's block scale S (from
// the largest m of its 8 pixels: |a| <= m); the LUT operand holds (2048 lo, hi) / T the same way (mkd_consts.hpp).  The
// two streams' values go through ONE v_cvt_scalef32_2xpk16_fp6_f32, which interleaves its two 16-value sources field by
// field (tools/micro/fp6_cross.hip).  A single-stream product reads the stream's three registers beside three zeros (the
// LUT registers opposite them may hold anything: e2m3 has no NaN or infinity); the merged tile reads all six.
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned v6u __attribute__((ext_vector_type(6)));
typedef int v8i __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void pool_harmonics_fp6(const f32x2 (&m)[4], const f32x2 (&c1)[4], const f32x2 (&s1)[4],
                                                   const unsigned char *brow, BFrag &g, f32x4 (&acc)[kUnfAccTiles]) {
    // the harmonic's two streams live in the conversion's first source, aq = (pk[0..3], qk[0..3]): the recurrence writes the
    // next harmonic into a fresh one (the k loop is unrolled: renaming, no copies)
    v16f aq, ap;
    f32x2 tc[4];
    auto pair = [](const v16f &v, int i) { return f32x2{v[2 * i], v[2 * i + 1]}; };
    auto put = [](v16f &v, int i, f32x2 x) { v[2 * i] = x.x; v[2 * i + 1] = x.y; };
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        put(aq, e, m[e] * c1[e]);
        put(aq, 4 + e, m[e] * s1[e]);
        tc[e] = c1[e] + c1[e];
    }
    // block scale S = 2^(exponent of the largest m) / 2: every |a| / S < 4 and every 2048 r / S < 4 (r < one f16 ulp of a)
    float mx = fmaxf(fmaxf(m[0].x, m[0].y), fmaxf(m[1].x, m[1].y));
    mx = fmaxf(mx, fmaxf(fmaxf(m[2].x, m[2].y), fmaxf(m[3].x, m[3].y)));
    const unsigned s_bits = (__float_as_uint(mx) & 0x7F800000u) - 0x00800000u;
    const float s_scale = __uint_as_float(s_bits);
    const int scale_b = (int)(s_bits >> 23) - 11;        // E8M0 of S / 2048
    float one = 1.f;
    asm("" : "+v"(one));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u32x4 hc, hs;
        v16f r16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x2 p = pair(aq, e), q = pair(aq, 4 + e);
            hc[e] = pack_rtz(p.x, p.y);
            hs[e] = pack_rtz(q.x, q.y);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x2 p = pair(aq, e), q = pair(aq, 4 + e);
            const f32x2 rc = {__builtin_fmaf(p.x, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(hc[e] & 0xffffu))),
                              __builtin_fmaf(p.y, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(hc[e] >> 16)))};
            const f32x2 rs = {__builtin_fmaf(q.x, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(hs[e] & 0xffffu))),
                              __builtin_fmaf(q.y, one, -(float)__builtin_bit_cast(_Float16, (unsigned short)(hs[e] >> 16)))};
            put(r16, e, rc * pk_set(2048.f));
            put(r16, 4 + e, rs * pk_set(2048.f));
        }
        // (written as inline assembly for its early-clobber destination: through the builtin, hipcc of ROCm 7.2 lets the six
        //  destination registers overlap a source that dies here -- v[36:41] <- v[16:31], v[32:47] -- and the instruction
        //  writes them while it still reads its thirty-two inputs: harmonics 2 and 3 came out with garbage cross terms)
        v6u d;
        asm("v_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, %3" : "=&v"(d) : "v"(aq), "v"(r16), "v"(s_scale));
        if (k < 2) {   // x_{k+1} = 2 c1 x_k - x_{k-1}, written over x_{k-1}; then the two change roles
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x2 p = pair(aq, e), q = pair(aq, 4 + e);
                put(ap, e, pk_fma(tc[e], p, k == 0 ? -m[e] : -pair(ap, e)));
                put(ap, 4 + e, k == 0 ? tc[e] * q : pk_fma(tc[e], q, -pair(ap, 4 + e)));
            }
            const v16f t = aq;
            aq = ap;
            ap = t;
        }
        const int a0 = 3 + 7 * k, u0 = 3 + 4 * k;
        const BFrag p0 = g, q0 = load_b(brow, u0 + 1), r = load_b(brow, u0 + 2), sf = load_b(brow, u0 + 3);
        if (k < 2) g = load_b(brow, u0 + 4);
        const f16x8 ch = __builtin_bit_cast(f16x8, hc), sh = __builtin_bit_cast(f16x8, hs);
        auto hh = [&](const BFrag &b, const f16x8 &st, f32x4 &c) {
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b.p0), st, c, 0, 0, 0);
        };
        // hi x hi: cos x P0 -> a0 | sin x P0, cos x Q0 -> a0+2 | sin x Q0 -> a0+1 | cos, sin x R -> a0+3, a0+4 | x S -> a0+5, a0+6
        hh(p0, ch, acc[a0 + 0]); hh(p0, sh, acc[a0 + 2]); hh(q0, sh, acc[a0 + 1]); hh(r, ch, acc[a0 + 3]);
        hh(r, sh, acc[a0 + 4]); hh(sf, ch, acc[a0 + 5]); hh(sf, sh, acc[a0 + 6]); hh(q0, ch, acc[a0 + 2]);
        // the cross terms: one instruction per accumulator; the LUT fragment's fourth word is its block scale
        v8i bc, bs, bm;      // (registers 6 and 7 of an fp6 operand are not read)
        bc[0] = (int)d[0]; bc[1] = (int)d[1]; bc[2] = (int)d[2]; bc[3] = 0; bc[4] = 0; bc[5] = 0;
        bs[0] = (int)d[3]; bs[1] = (int)d[4]; bs[2] = (int)d[5]; bs[3] = 0; bs[4] = 0; bs[5] = 0;
        bm[0] = (int)d[0]; bm[1] = (int)d[1]; bm[2] = (int)d[2]; bm[3] = (int)d[3]; bm[4] = (int)d[4]; bm[5] = (int)d[5];
        auto single = [&](const u32x4 &f, const v8i &b, f32x4 &c) {
            v8i a;   // the fragment's own four registers; what follows them meets the zeros of b
            a[0] = (int)f[0]; a[1] = (int)f[1]; a[2] = (int)f[2]; a[3] = (int)f[3];
            c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 2, 2, 0, (int)f[3], 0, scale_b);
        };
        single(p0.p1, bc, acc[a0 + 0]);
        single(q0.p1, bs, acc[a0 + 1]);
        {   // cos x Q0 + sin x P0 (P0 and Q0 carry the same scale)
            v8i a;
            a[0] = (int)q0.p1[0]; a[1] = (int)q0.p1[1]; a[2] = (int)q0.p1[2];
            a[3] = (int)p0.p1[0]; a[4] = (int)p0.p1[1]; a[5] = (int)p0.p1[2];
            acc[a0 + 2] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, bm, acc[a0 + 2], 2, 2, 0, (int)p0.p1[3], 0, scale_b);
        }
        single(r.p1, bc, acc[a0 + 3]);
        single(r.p1, bs, acc[a0 + 4]);
        single(sf.p1, bc, acc[a0 + 5]);
        single(sf.p1, bs, acc[a0 + 6]);
    }
}

// Unfolded form: the 24 accumulator tiles of the row loop -> the 21 tiles of packed output columns (mkd_consts.hpp):
//   relcos_k = cos x EPc - sin x EPs, relsin_k = sin x EPc + cos x EPs (columns 0-15 in P0 / Q0, 16-24 in slots 0-8 of R / S),
//   abscos_k / abssin_k = the EC columns: 0-6 in slots 9-15 of R, 7-8 in slots 9-10 of S.
// Slot of (lane, i) in a tile: 4 (lane >> 4) + i.  Unused slots are set to zero (the norms run over whole tiles).
__device__ __forceinline__ void combine_tiles(const f32x4 (&a)[kUnfAccTiles], int q, f32x4 (&o)[kTiles]) {
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int b = 3 + 7 * h, l = 3 + 6 * h;
        o[l + 0] = a[b + 0] - a[b + 1];
        o[l + 1] = a[b + 2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int slot = 4 * q + i;
            const bool lo9 = slot < 9, s910 = slot == 9 || slot == 10;
            o[l + 2][i] = a[b + 3][i] - (lo9 ? a[b + 6][i] : 0.f);   // cos x R - sin x S
            o[l + 3][i] = a[b + 4][i] + (lo9 ? a[b + 5][i] : 0.f);   // sin x R + cos x S
            o[l + 4][i] = s910 ? a[b + 5][i] : 0.f;
            o[l + 5][i] = s910 ? a[b + 6][i] : 0.f;
        }
    }
}

// which block of the raw descriptor a packed tile's slots belong to (normalize.glsl: polar | cartesian):
// 0 = all polar, 1 = all cartesian (or unused = 0), 2 = mixed: the first slots polar (folded: 10, unfolded: 9), the others cartesian
// (one rule for both forms: folded tile 3 + 6h + 2 (LUT tile) + (U | V), unfolded tile 3 + 6h + part)
__device__ __forceinline__ constexpr int tile_block(int t) {
    if (t < 3) return t == 0 ? 0 : (t == 1 ? 2 : 1);
    const int part = (t - 3) % 6;
    return part < 2 ? 0 : (part < 4 ? 2 : 1);
}

// Epilogue, per wave and batch: acc[t][i] holds the pooled sum of packed column 16t + 4q + i for the lane's
// own patch.  normalize.glsl:22-142 (polar | cartesian | all), whitening.glsl:22-77 as an MFMA with the
// accumulators as B operand (out^T = W_T x raw, the mean folded into a bias), normalize_final.glsl.
// Whitening fragments (host: mkd_consts.cpp): f16: [step 11][row tile 8][hi|lo][lane][8], step s covers
// accumulator tiles 2s, 2s+1; f32: [tile 21][i 4][row tile 8][lane].
// f16 path: on entry step 0 of the fragments is on its way into its slot (requested by the caller during patch row 31);
// on exit LUT row 0 of the next batch is on its way into row buffer 0 if `more`.  Every wave of the workgroup must call.
template <int POOL, int W>
__device__ __forceinline__ void finish_descriptors(const f32x4 (&acc_row)[acc_tiles(fold_form(POOL))], int lane, int wave, bool valid,
                                                   long patch, const short *__restrict__ colmap,
                                                   const unsigned char *__restrict__ wfrag,
                                                   const float *__restrict__ bias, float *__restrict__ out,
                                                   float *__restrict__ raw_out, unsigned char *s_mem,
                                                   const unsigned char *__restrict__ lut_rows, bool more) {
    constexpr bool kFold = fold_form(POOL);
    const int q = lane >> 4;
    f32x4 acc[kTiles];
    if constexpr (kFold) {   // the accumulators are the packed tiles
#pragma unroll
        for (int t = 0; t < kTiles; ++t) acc[t] = acc_row[t];
    } else {
        combine_tiles(acc_row, q, acc);
    }
    if constexpr (f16_family(POOL)) {
        __syncthreads();   // every wave has left patch row 31: row buffer 1 is free too
        issue_w_step<W>(wfrag, 1, s_mem, wave, lane);
        issue_w_step<W>(wfrag, 2, s_mem, wave, lane);
    }
    // mixed tiles hold polar kernels in their first packed columns (0-9; unfolded: 0-8) and cartesian ones in the others
    bool lo9[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) lo9[i] = 4 * q + i < (kFold ? kPolarSlots : 9);
    float sp = 0.f, sc = 0.f;
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (tile_block(t) == 2) {
                const float v2 = acc[t][i] * acc[t][i];
                sp += lo9[i] ? v2 : 0.f;
                sc += lo9[i] ? 0.f : v2;
            } else if (tile_block(t) == 0) {
                sp = fmaf(acc[t][i], acc[t][i], sp);
            } else {
                sc = fmaf(acc[t][i], acc[t][i], sc);
            }
        }
    sp += __shfl_xor(sp, 16); sp += __shfl_xor(sp, 32);
    sc += __shfl_xor(sc, 16); sc += __shfl_xor(sc, 32);
    const float inv_p = 1.f / __builtin_amdgcn_sqrtf(sp), inv_c = 1.f / __builtin_amdgcn_sqrtf(sc);
    // normalize.glsl then L2-normalises the concatenation of the two unit blocks.  Its squared norm follows from the
    // block sums (sp inv_p^2 + sc inv_c^2, within 2 ulp of the shader's second pass over the 238 values), so the two
    // scalings fold into one pass
    const float sa = fmaf(sp * inv_p, inv_p, (sc * inv_c) * inv_c);
    const float inv_a = 1.f / __builtin_amdgcn_sqrtf(sa);
    const float k_p = inv_p * inv_a, k_c = inv_c * inv_a;
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool polar = tile_block(t) == 0 || (tile_block(t) == 2 && lo9[i]);
            acc[t][i] *= polar ? k_p : k_c;
        }
    if (raw_out) {  // verification tap: the 238-D descriptor before whitening
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = colmap[t * 16 + 4 * q + i];   // (-2 - d: the column holds minus entry d -- the folded forms)
                if (valid && d != -1) raw_out[patch * 238 + (d >= 0 ? d : -2 - d)] = d >= 0 ? acc[t][i] : -acc[t][i];
            }
    }
    f32x4 o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (f16_family(POOL)) {
        // The whitening is bound by operand delivery (each wave needs all 176 KiB of fragments per batch): from LDS, where
        // the 8 waves share one copy, they arrive at twice the rate the vector L1 gives each wave its own.
        constexpr int kDma = 16 / W;   // DMA instructions per lane and step
        if (raw_out) wait_vmcnt<0>();  // stores and loads retire out of order with respect to each other
        // Within a wave the LDS reads run one unit (4 row tiles, hi + lo = 8 KiB) ahead of the MFMAs, in two register
        // buffers: the waves of a workgroup move in lock step here, so without that the LDS and the matrix pipe would
        // take turns idling.
        u32x4 wbuf[2][8];   // [buffer][row tile rr][hi|lo]
        auto read_unit = [&](int u, u32x4 (&dst)[8]) {
            const u32x4 *w = reinterpret_cast<const u32x4 *>(s_mem + wstage_slot(u >> 1)) + (u & 1) * 8 * 64 + lane;
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[j] = w[j * 64];
        };
        f16x8 yh, yl;
        auto mma_unit = [&](int u, const u32x4 (&src)[8]) {
            const int r0 = (u & 1) * 4;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                o[r0 + rr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, src[2 * rr + 1]), yh, o[r0 + rr], 0, 0, 0);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                o[r0 + rr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, src[2 * rr]), yl, o[r0 + rr], 0, 0, 0);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                o[r0 + rr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, src[2 * rr]), yh, o[r0 + rr], 0, 0, 0);
        };
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            // own share of step s has landed (steps s+1, and s+2 for s = 0, may still be in flight) and own reads of
            // step s-1 have returned; after the barrier that holds for every wave, so the slot of step s-1 can take
            // step s+2
            if (s == 0) wait_vmcnt<2 * kDma>();
            else if (s < 10) wait_vmcnt<kDma>();
            else wait_vmcnt<0>();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __syncthreads();
            if (s >= 1 && s + 2 < 11) issue_w_step<W>(wfrag, s + 2, s_mem, wave, lane);
            if (s == 10 && more) issue_lut_row<W, kFold, valu_odd_cart(POOL)>(lut_rows, 0, s_mem, wave, lane);
            read_unit(2 * s, wbuf[0]);
            __builtin_amdgcn_sched_barrier(0);
            if (s > 0) mma_unit(2 * s - 1, wbuf[1]);
            {
                const f32x4 y0 = acc[2 * s];
                const f32x4 y1 = 2 * s + 1 < kTiles ? acc[(2 * s + 1 < kTiles) ? 2 * s + 1 : 0] : f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x2 y[4] = {{y0[0], y0[1]}, {y0[2], y0[3]}, {y1[0], y1[1]}, {y1[2], y1[3]}};
                AFrag<LF_POOL_F16X3> yb;
                yb.set(y);
                yh = __builtin_bit_cast(f16x8, yb.hi);
                yl = __builtin_bit_cast(f16x8, yb.lo);
            }
            __builtin_amdgcn_sched_barrier(0);
            read_unit(2 * s + 1, wbuf[1]);
            __builtin_amdgcn_sched_barrier(0);
            mma_unit(2 * s, wbuf[0]);
            __builtin_amdgcn_sched_barrier(0);
        }
        mma_unit(21, wbuf[1]);
    } else {
        const float *w = reinterpret_cast<const float *>(wfrag);
        float wbuf[2][16];  // unit = two (tile, i) steps x 8 row tiles
        auto load_unit = [&](int u, float (&dst)[16]) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int r = 0; r < 8; ++r) dst[k * 8 + r] = w[((2 * u + k) * 8 + r) * 64 + lane];
        };
        load_unit(0, wbuf[0]);
#pragma unroll
        for (int u = 0; u < 42; ++u) {
            if (u + 1 < 42) load_unit(u + 1, wbuf[(u + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ti = 2 * u + k;
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    o[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wbuf[u & 1][k * 8 + r], acc[ti >> 2][ti & 3], o[r], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // lane holds outputs 16r + 4q + i of its patch: add the bias (-W mean), L2-normalise, store
    float ss = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(bias + 16 * r + 4 * q);
        o[r] += b;
#pragma unroll
        for (int i = 0; i < 4; ++i) ss = fmaf(o[r][i], o[r][i], ss);
    }
    ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);
    const float inv = 1.f / __builtin_amdgcn_sqrtf(ss);   // one division, 32 multiplications: 1 ulp from 32 divisions
    if (valid) {
#pragma unroll
        for (int r = 0; r < 8; ++r) *reinterpret_cast<f32x4 *>(out + patch * 128 + 16 * r + 4 * q) = o[r] * inv;
    }
}

// ---- keypoint mode (SRC = kSrcKeypoints) --------------------------------------------------------------------------
// What the describe kernel is given instead of patches: the pyramids (mkd_pyramid.hip) and the keypoint list.
struct KpSource {
    const float *pyr;            // pyramids of the frames, pyr_stride floats apart
    long pyr_stride;
    const float *kps;            // [n][5] x, y, size, angle (degrees), response
    const unsigned *frame_of;    // [n] frame of each keypoint, or null: all on frame 0
    unsigned n_frames;           // frames in the store: larger indices (caller's data) are clamped
    float psf;                   // patch_scale_factor
    PyramidDesc pd;
    // row-split form only: workgroups per batch (2 or 4), the partial sums' exchange buffer
    // [batch][role R-1][wave W][tile 21][half 2][lane 64] 2 x f32, its arrival counters [batch][wave] and an error word
    int split;
    float *xchg;
    unsigned *xchg_cnt;
};

// Batches of a workgroup.  Keypoints arrive ordered by frame, and every XCD has its own L2: workgroups that share an XCD
// (b, b + 8, ...: dispatch is round-robin over the 8 XCDs -- a matter of speed only, nothing depends on it) walk ONE
// contiguous eighth of the batches, so that a frame's pyramid is fetched into one L2 instead of eight.
struct BatchWalk { long cur, end, step; };
__device__ __forceinline__ BatchWalk kp_batches(long nbatch) {
    const long g = gridDim.x, b = blockIdx.x;
    if ((g & 7) == 0 && nbatch > g) {
        const long chunk = (nbatch + 7) / 8, lo = (b & 7) * chunk, hi = lo + chunk < nbatch ? lo + chunk : nbatch;
        return BatchWalk{lo + (b >> 3), hi, g >> 3};
    }
    return BatchWalk{b, nbatch, g};
}

__device__ __forceinline__ int readlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// A producer wave: samples the patches of ITS describe wave (wave pw of the workgroup's W describe waves) into that wave's
// row ring, patch_gradients.glsl:42-70 with the arithmetic of mkd_sample.h.
// Work unit = a quarter of a row group: rows 4G..4G+3 of patches 4q..4q+3, as eight blocks of 4 rows x 16 pixels -- one
// block per load instruction, lane = (row r = lane >> 4, column c = lane & 15): a compact footprint of a few cache lines
// (the texture path's cost is per line touched per instruction: a whole patch row per instruction, which the ring's row
// order would suggest, costs 7x as much -- tools/micro/gather_patterns.hip).  One quarter per row step of the describe
// waves: quarter Q = g + 7 is written during step g, i.e. a group is complete one barrier before its first row is read and
// is written into the slots of rows read for the last time one barrier earlier (ring of 12, see kRingSlotsKp).  Quarters
// 32..38 are the first seven of the workgroup's NEXT batch; the epilogue of the describe waves is a pause.
// The taps of a quarter are requested one step BEFORE it is written (two register sets, the step loop unrolled by two):
// their latency passes beside the previous quarter's arithmetic instead of in front of the barrier.
// Every barrier of the describe waves has its twin here: 32 row steps + 12 in finish_descriptors per batch.
// The producers also request the LUT rows of the row loop: an LDS-DMA request stalls its issuer for 60-180 cycles, which a
// producer can afford, so a describe wave issues no memory instruction between its barriers.
struct KpTaps { f32x2 top[8], bot[8]; float ax[8], ay[8]; };

// min(max(x, 0), hi) for hi >= 0 as ONE instruction (the median of x, 0, hi); hipcc cannot fuse the pair itself because it
// does not know hi >= 0
__device__ __forceinline__ int clamp_med3(int x, int hi) {
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(hi));
    return r;
}

// (uniform base) + (unsigned 32-bit lane offset) -> global_load_dwordx2 v, v_off, s[base:base+1]: no 64-bit address arithmetic
// (the two empty asm statements: see lds_dma16_sv).  Texel addresses are 4-byte aligned only.
__device__ __forceinline__ f32x2 load2_sv(const unsigned char *uniform_base, unsigned lane_off) {
    asm("" : "+s"(uniform_base));
    asm volatile("" : "+v"(lane_off));
    typedef f32x2 f32x2_a4 __attribute__((aligned(4)));
    return *reinterpret_cast<const __attribute__((address_space(1))) f32x2_a4 *>(
        (const __attribute__((address_space(1))) unsigned char *)uniform_base + lane_off);
}

// The sampling machinery of one row ring: the geometry of the ring's keypoints and the two halves of a quarter's work.
template <int W>
struct KpSampler {
    const KpSource &ks;
    const LevelTable &lt;
    const long *lvl_offset;
    long n;
    unsigned char *ring;
    int pw, lane, r, c;
    // geometry of a batch's 16 keypoints, one per lane: lanes 0-15 hold set 0, lanes 16-31 set 1 (this batch / the next).
    // g_xmax / g_ymax: largest first-tap index in the level's allocation (apron included); the row pitch is g_xmax + 2
    // texels and the apron kPyrApron on every level, so neither needs a register of its own.
    float g_ca = 0.f, g_sa = 0.f, g_rem = 0.f, g_cx = 0.f, g_cy = 0.f;
    int g_xmax = 0, g_ymax = 0, g_cov = 0;
    unsigned g_lo = 0, g_hi = 0;

    __device__ __forceinline__ KpSampler(const KpSource &ks_, const LevelTable &lt_, const long *lvl_offset_, long n_,
                                         unsigned char *s_mem, int pw_, int lane_)
        : ks(ks_), lt(lt_), lvl_offset(lvl_offset_), n(n_), ring(s_mem + kRingOff + pw_ * (kRingSlotsKp * 2048)), pw(pw_),
          lane(lane_), r(lane_ >> 4), c(lane_ & 15) {}

    __device__ __forceinline__ void load_geometry(long batch, int set) {
        long k = batch * (16 * W) + pw * 16 + (lane & 15);
        k = k < n ? k : n - 1;
        const float *kp = ks.kps + k * 5;
        const KpGeom g = keypoint_geometry(kp[0], kp[1], kp[2], kp[3], ks.psf, lt);
        // first texel of the level's allocation (apron included): offsets from it are never negative
        const int a = lt.apron[g.level], pitch = lt.pitch[g.level];
        const float *a0 = ks.pyr + (ks.frame_of ? (long)min(ks.frame_of[k], ks.n_frames - 1u) * ks.pyr_stride : 0L) +
                          lvl_offset[g.level] -
                          (long)a * pitch - a;
        if ((lane >> 4) == set) {
            g_ca = g.ca; g_sa = g.sa; g_rem = g.rem; g_cx = g.cx; g_cy = g.cy;
            g_xmax = lt.w[g.level] + 2 * a - 2; g_ymax = lt.h[g.level] + 2 * a - 2;   // (pitch = w + 2a, a = kPyrApron)
            g_cov = g.covered ? 1 : 0;
            g_lo = (unsigned)(uintptr_t)a0; g_hi = (unsigned)((uintptr_t)a0 >> 32);
        }
    }
    __device__ __forceinline__ const unsigned char *base_of(int src) const {
        return reinterpret_cast<const unsigned char *>((uintptr_t)(unsigned)readlane_i((int)g_lo, src) |
                                                       ((uintptr_t)(unsigned)readlane_i((int)g_hi, src) << 32));
    }
    // requests the taps of a quarter (fetch_covered of mkd_sample.h: indices clamped into the level's allocation)
    __device__ __forceinline__ void request(int quarter, int set, KpTaps &t) const {
        if constexpr (ablate::kNoProducer) return;
        const int q = quarter & 3, ly = 4 * (quarter >> 2) + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int src = 16 * set + 4 * q + i;   // uniform
            const float ca = readlane_f(g_ca, src), sa = readlane_f(g_sa, src), rem = readlane_f(g_rem, src);
            const float cx = readlane_f(g_cx, src), cy = readlane_f(g_cy, src);
            const int xmax = readlane_i(g_xmax, src), ymax = readlane_i(g_ymax, src), pitch4 = 4 * (xmax + 2);
            constexpr int apron = kPyrApron;
            const unsigned char *a0 = base_of(src), *a1 = a0 + pitch4;   // the two tap rows: two uniform bases, one lane offset
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const SamplePos p = sample_position(ca, sa, rem, cx, cy, 16 * hh + c, ly);
                t.ax[2 * i + hh] = p.ax;
                t.ay[2 * i + hh] = p.ay;
                // the apron goes onto both coordinates as ONE two-wide float addition (exact: integers far below 2^23)
                typedef float v2 __attribute__((ext_vector_type(2)));
                const v2 fa = v2{p.fx0, p.fy0} + v2{(float)apron, (float)apron};
                const int ix = clamp_med3((int)fa.x, xmax), iy = clamp_med3((int)fa.y, ymax);
                const unsigned off = __umul24((unsigned)iy, (unsigned)pitch4) + 4u * (unsigned)ix;   // both < 2^24: full-rate multiply
                if constexpr (ablate::kNoTaps) {
                    t.top[2 * i + hh] = f32x2{__uint_as_float(off), p.ax};
                    t.bot[2 * i + hh] = f32x2{p.ay, (float)pitch4};
                    continue;
                }
                t.top[2 * i + hh] = load2_sv(a0, off);
                t.bot[2 * i + hh] = load2_sv(a1, off);
            }
        }
    }
    // blends them and writes the quarter's rows into the ring
    __device__ __forceinline__ void finish(int quarter, int set, int slot0, const KpTaps &t) const {
        if constexpr (ablate::kNoProducer) return;
        const int G = quarter >> 2, q = quarter & 3;
        // (slot0 + 4G) mod 12 is a multiple of 4: the group's four rows sit in consecutive slots.  Ring slot layout:
        // [half 2][16-byte chunk of the half-row 4][patch 16][4 pixels]; this lane's pixel c (+16) of patch 4q + i
        unsigned char *dst = ring + ((slot0 + 4 * G) % kRingSlotsKp + r) * 2048 + (c & 3) * 4 + (c >> 2) * 256 + q * 64;
        int any_uncovered = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            any_uncovered |= 1 - readlane_i(g_cov, 16 * set + 4 * q + i);
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int k = 2 * i + hh;
                *reinterpret_cast<float *>(dst + hh * 1024 + i * 16) =
                    bilinear_blend(t.top[k].x, t.top[k].y, t.bot[k].x, t.bot[k].y, t.ax[k], t.ay[k]);
            }
        }
        // keypoints whose footprint leaves the apron (centre outside the frame, sizes beyond the pyramid, non-finite data):
        // rare -- their samples are redone with MirroredRepeat evaluated per tap
        if (any_uncovered) {
            const int ly = 4 * G + r;
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                const int src = 16 * set + 4 * q + i;
                if (readlane_i(g_cov, src)) continue;
                constexpr int apron = kPyrApron;
                const int pitch = readlane_i(g_xmax, src) + 2;
                const int w = readlane_i(g_xmax, src) + 2 - 2 * apron, h = readlane_i(g_ymax, src) + 2 - 2 * apron;
                const float *lvl0 = reinterpret_cast<const float *>(base_of(src)) + (long)apron * pitch + apron;
#pragma unroll 1
                for (int hh = 0; hh < 2; ++hh) {
                    const SamplePos p = sample_position(readlane_f(g_ca, src), readlane_f(g_sa, src), readlane_f(g_rem, src),
                                                        readlane_f(g_cx, src), readlane_f(g_cy, src), 16 * hh + c, ly);
                    const Taps tm = fetch_mirrored(lvl0, w, h, pitch, p);
                    *reinterpret_cast<float *>(dst + hh * 1024 + i * 16) =
                        bilinear_blend(tm.t00, tm.t10, tm.t01, tm.t11, p.ax, p.ay);
                }
            }
        }
    }
};

template <int W>
__device__ __forceinline__ void kp_produce(const KpSource &ks, const LevelTable &lt, const long *lvl_offset, long n,
                                           BatchWalk walk, unsigned char *s_mem, const unsigned char *__restrict__ lut_rows,
                                           int pw, int lane) {
    // The producer is the shorter instruction stream of the two waves on its SIMD, but its step ends in the barrier the
    // describe waves of all four SIMDs wait at: served first, it keeps out of their way (same-box A/B: +4 %)
    __builtin_amdgcn_s_setprio(ablate::kProducerPrio);
    KpSampler<W> sm(ks, lt, lvl_offset, n, s_mem, pw, lane);
    KpTaps ta, tb;
    int set = 0, slot0 = 0;
    // the first seven quarters of the first batch, before the describe waves' first row barrier.  (Two tap sets in flight
    // here, as in kp_produce_split, was measured in round 6: 76.5 / 79.2 / 93.0 us against 76.9 / 78.7 / 93.6 at 6000 / 8192 /
    // 10 000 keypoints -- nothing.  Letting the describe
    // waves, idle until then, sample every other one of them was tried: nothing to gain -- same-box, a one-round launch of
    // 10 000 keypoints took 96 us either way.)
    sm.load_geometry(walk.cur, 0);
#pragma unroll 1
    for (int quarter = 0; quarter < 7; ++quarter) {
        sm.request(quarter, 0, ta);
        sm.finish(quarter, 0, 0, ta);
    }
    sm.request(7, 0, ta);
#pragma unroll 1
    for (long batch = walk.cur; batch < walk.end; batch += walk.step) {
        const bool more = batch + walk.step < walk.end;
        if (more) sm.load_geometry(batch + walk.step, set ^ 1);
        const int slot1 = (slot0 + 8) % kRingSlotsKp;
        // step g: LUT row g + 1 is requested into the row buffer the describe waves have just left (row g uses buffer g & 1),
        // then the taps of the quarter step g + 1 will write (vector-memory results return in issue order: the taps, which
        // have a whole step, queue behind the LUT pieces, not the other way round); then the quarter of THIS step, whose
        // taps landed during the previous one, is blended and written
        auto step = [&](int g, KpTaps &cur, KpTaps &nxt) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // ring writes, LUT pieces and taps have landed
            __syncthreads();
            if (g < 31) issue_lut_row<W, true, true>(lut_rows, g + 1, s_mem + ((g + 1) & 1) * kRowBytes, pw, lane);
            const int qn = g + 8;    // the quarter of step g + 1
            if (qn < 32) sm.request(qn, set, nxt);
            else if (more) sm.request(qn - 32, set ^ 1, nxt);   // (g = 31: quarter 7 of the next batch)
            __builtin_amdgcn_sched_barrier(0);
            const int qc = g + 7;
            if (qc < 32) sm.finish(qc, set, slot0, cur);
            else if (more) sm.finish(qc - 32, set ^ 1, slot1, cur);
        };
#pragma unroll 1
        for (int g = 0; g < ablate::kRows; g += 2) {
            step(g, ta, tb);
            step(g + 1, tb, ta);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll 1
        for (int e = 0; e < 12; ++e) __syncthreads();   // finish_descriptors: one on entry, one per whitening step
        set ^= 1;
        slot0 = slot1;
    }
}

// The row-split form's share of a batch: patch rows [lo, hi) of its 32 keypoints.  The describe waves need blurred rows
// lo-1 .. hi, i.e. raw rows lo-3 .. hi+2 (clamped to the patch): the row groups of four that hold them are the quarters
// [q_first, q_end) of the producers' numbering (quarter = 4 x group + patch quad).  n_pro of them are sampled before the
// first row barrier: the describe waves' first step reads raw rows up to lo+3 and the second up to lo+4, so from the group
// of row lo+4 on a group has exactly the four steps before its first use -- everything before it, and all but one quarter
// of that group when lo > 0 (its first use comes one step after the start), belongs to the prologue: 7 quarters for the
// rows from 0 (as in the whole-patch form), 11 otherwise.  Ring slot of raw row r: r mod 12, as in the whole-patch form.
struct RowSpan {
    int lo, hi, q_first, q_end, n_pro;
    bool consumer;      // the workgroup of the LAST rows: it collects the others' partial sums and finishes the descriptors
};
__device__ __forceinline__ RowSpan row_span(int role, int n_roles) {
    RowSpan sp;
    sp.lo = 32 * role / n_roles;
    sp.hi = 32 * (role + 1) / n_roles;
    const int r_first = sp.lo - 3 > 0 ? sp.lo - 3 : 0, r_last = sp.hi + 2 < 31 ? sp.hi + 2 : 31;
    sp.q_first = 4 * (r_first >> 2);
    sp.q_end = 4 * ((r_last >> 2) + 1);
    sp.n_pro = sp.lo == 0 ? 7 : 11;
    sp.consumer = role == n_roles - 1;
    return sp;
}

// The producer wave of a row-split workgroup: kp_produce for rows [lo, hi) of ONE batch.  One quarter per row step of the
// describe waves, requested a step ahead like there; every barrier of the describe waves has its twin here: hi - lo row steps,
// and the 12 of finish_descriptors in the consumer workgroup.
template <int W>
__device__ __forceinline__ void kp_produce_split(const KpSource &ks, const LevelTable &lt, const long *lvl_offset, long n,
                                                 long batch, const RowSpan &sp, unsigned char *s_mem,
                                                 const unsigned char *__restrict__ lut_rows, int pw, int lane) {
    __builtin_amdgcn_s_setprio(ablate::kProducerPrio);
    KpSampler<W> sm(ks, lt, lvl_offset, n, s_mem, pw, lane);
    KpTaps ta, tb;
    sm.load_geometry(batch, 0);
    // the prologue, two tap sets in flight: the taps of quarter i + 1 are on their way while quarter i is blended
    sm.request(sp.q_first, 0, ta);
#pragma unroll 1
    for (int i = 0; i + 1 < sp.n_pro; i += 2) {
        sm.request(sp.q_first + i + 1, 0, tb);
        sm.finish(sp.q_first + i, 0, 0, ta);
        sm.request(sp.q_first + i + 2, 0, ta);     // (n_pro is odd: i + 2 <= n_pro - 1 is a prologue quarter)
        sm.finish(sp.q_first + i + 1, 0, 0, tb);
    }
    sm.finish(sp.q_first + sp.n_pro - 1, 0, 0, ta);
    const int q_step0 = sp.q_first + sp.n_pro;      // the quarter row step 0 writes
    if (q_step0 < sp.q_end) sm.request(q_step0, 0, ta);
    auto step = [&](int st, KpTaps &cur, KpTaps &nxt) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // ring writes, LUT pieces and taps have landed
        __syncthreads();
        // LUT row lo + st + 1 into the buffer the describe waves have just left (never beyond the span: during the last
        // step of the consumer workgroup buffer 0 takes the epilogue's first whitening step)
        if (sp.lo + st + 1 < sp.hi) issue_lut_row<W, true, true>(lut_rows, sp.lo + st + 1, s_mem + ((st + 1) & 1) * kRowBytes, pw, lane);
        if (q_step0 + st + 1 < sp.q_end) sm.request(q_step0 + st + 1, 0, nxt);
        __builtin_amdgcn_sched_barrier(0);
        if (q_step0 + st < sp.q_end) sm.finish(q_step0 + st, 0, 0, cur);
    };
#pragma unroll 1
    for (int st = 0; st < sp.hi - sp.lo; st += 2) {
        step(st, ta, tb);
        step(st + 1, tb, ta);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (sp.consumer) {
#pragma unroll 1
        for (int e = 0; e < 12; ++e) __syncthreads();   // finish_descriptors: one on entry, one per whitening step
    }
}

constexpr int kSplitSpinMax = 1 << 21;   // polls of a consumer wave for its partners' partial sums before it gives up (~1 s)

}  // namespace

// grid = min(#batches, #CUs) persistent workgroups of 8 waves; a batch is 128 patches (16 per wave).
// Per patch row g (32 per batch): one barrier, after which the LUT row g is in LDS (issued a whole row
// earlier, double-buffered) and every wave has left row g-1.  Raw patch rows arrive by LDS-DMA into a
// 6-slot ring private to each wave, one row per step, so the main loop holds no patch data in VGPRs beyond
// the three blurred rows of the gradient stencil.
// Algorithmic HBM bytes per patch: 4096 read + 512 written; the kernel moves nothing else.
// W = waves per workgroup: 8 (128 patches, two waves per SIMD) for throughput; 4 (64 patches) when the whole request
// fits one round of workgroups anyway, so that it spreads over twice as many CUs with a SIMD to each wave.
// SRC = kSrcKeypoints (keypoint mode, f16x3 pooling): the workgroup has 2 W waves.  Waves 0 .. W-1 are the describe waves
// of the text above; waves W .. 2W-1 are their producers (kp_produce): wave W + i samples the patches of describe wave i from
// the pyramid straight into its row ring, so a sampled patch never leaves the CU.  `patches` is unused, `ks` says what to
// sample.  The two kinds of wave sit side by side on every SIMD -- one waits on the texture path while the other computes.
// SRC = kSrcKeypointsSplit (W = 2; requests small enough that every workgroup below is resident at once): a launch of the
// form above is a wave walking 32 rows for its 16 patches whatever the request's size -- ~70 us of latency at the reference's
// own 2000-3000 keypoints, on a quarter of the chip.  Here R = 2 or 4 workgroups share a batch of 32 keypoints by ROWS:
// workgroup `role` samples and pools rows [32 role / R, 32 (role + 1) / R) only (pooling is a sum over pixels), the first
// R - 1 leave their 21 accumulator tiles in global memory and count themselves in, the last one -- the highest workgroup id of
// the batch, so that those it waits for were dispatched before it -- adds them to its own in a fixed order and runs the
// epilogue.  A descriptor's sum is then R partial chains instead of one: bit-identical within the form, ~1e-7 relative
// from the whole-patch forms.  Same sampling, blur, gradient and MFMA arithmetic per row.
template <int ANGLE, int POOL, int W, int SRC>
__global__ __launch_bounds__(SRC != kSrcPatches ? 128 * W : 64 * W) void mkd_pool(
    const float *__restrict__ patches, long n_host, const unsigned long long *__restrict__ n_dev,
    const unsigned char *__restrict__ lut_rows, const short *__restrict__ colmap, const unsigned char *__restrict__ wfrag,
    const float *__restrict__ bias, const float *__restrict__ odd_cart, float *__restrict__ out, float *__restrict__ raw_out,
    std::conditional_t<SRC != kSrcPatches, KpSource, unsigned *> ks, unsigned long long *__restrict__ clk) {
    constexpr bool kKp = SRC != kSrcPatches, kSplit = SRC == kSrcKeypointsSplit;
    // Patch mode, 8 waves: `ks` is the launch's claim counter (zero on entry), or null.  With a counter only a workgroup's
    // FIRST batch is its id; every later one is gridDim.x + a ticket drawn from the counter at run time, so that a workgroup
    // which runs late (a late start, a slower CU) ends up with fewer batches instead of holding the launch's end up
    // (launch_describe says which launches claim; the batch loop below, how).  Null, and in every other form: the static
    // walk, batch b + k gridDim.x in turn k.
    // (LF_POOL_F32, the verification mode, stays static: its 8-wave form spills already, and the claim costs it two registers more)
    constexpr bool kClaimForm = SRC == kSrcPatches && W == 8 && f16_family(POOL);
    static_assert(!kSplit || W == 2, "the row-split form is the narrow (2 + 2 wave) form");
    // clk (LF_MKD_FLAG_KERNEL_TIMING, else null): workgroup 0 stamps the shader clock (s_memtime) and the constant 100 MHz
    // clock (s_memrealtime) on entry and on exit -- the clock the chip sustained under THIS launch is their quotient
    // (MI355X_MICROARCH.md, DVFS give-back); the values go to a buffer nothing else reads
    if (clk && blockIdx.x == 0 && threadIdx.x == 0) {
        clk[0] = __builtin_readcyclecounter();
        clk[1] = __builtin_amdgcn_s_memrealtime();
    }
    [[maybe_unused]] ablate::WgClock wg_clock;   // (instrument builds only: tools/wg_spread.py)
    if constexpr (!kKp) wg_clock.enter(out, n_host);
    constexpr int kSlots = kKp ? kRingSlotsKp : kRingSlots;
    static_assert(!kKp || POOL == LF_POOL_F16X3, "keypoint mode pools in f16x3");
    constexpr int kMPool = POOL == LF_POOL_F16_FP6 ? LF_POOL_F16X3 : POOL;   // the m stream keeps the three-term form
    constexpr bool kFold = fold_form(POOL), kOddV = valu_odd_cart(POOL);
    // Patch mode, f16x3: the middle rows go in pairs over fixed ring slots (see patch_row).  LF_POOL_F32 and LF_POOL_F16_FP6
    // keep the one-row body and its rotating slots: with the pair body their 8-wave forms need 290-420 bytes of scratch a lane.
    constexpr bool kPairs = SRC == kSrcPatches && POOL == LF_POOL_F16X3;
    static_assert(!kKp || (kFold && kOddV), "the producers write the folded forms' LDS map and request f16x3's LUT pieces");
    constexpr int kNAcc = acc_tiles(kFold), kRowB = row_bytes(kFold), kRingO = ring_off(kFold);
    __shared__ __attribute__((aligned(16))) unsigned char s_mem[kRingO + W * kSlots * 2048 +
                                                                (kKp ? kLevelTableBytes + kMaxPyrLevels * 8 : 0) +
                                                                (kClaimForm ? 16 : 0)];
    // claim forms: the word behind the rings through which wave 0 hands the workgroup's latest ticket to the other waves
    // (an LDS pointer by type: through a generic one the accesses are flat instructions, which count on vmcnt as well)
    typedef volatile __attribute__((address_space(3))) unsigned lds_ticket;
    [[maybe_unused]] lds_ticket *ticket_word = (lds_ticket *)((lds_u8 *)s_mem + (kRingO + W * kSlots * 2048));
    // number of patches: given by the host, or (graph-captured pipelines) left on the device by the previous stage
    const long n = n_dev ? (long)*n_dev : n_host;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 15, q = lane >> 4;
    const int addr_l = ((lane - 16) & 63) * 4, addr_r = ((lane + 16) & 63) * 4;
    const bool has_l = q > 0, has_r = q < 3;
    // The pair forms' halo records (hblur_row_fold_rec): wave w's 2 KiB area is the w-th of the eight holes that the x-odd
    // cartesian tiles leave in the two LUT row buffers -- pieces 6 j + 4, 6 j + 5 of a buffer, which issue_lut_row<ODDV>
    // never requests and the row loop never reads (the LDS map, says why nothing else touches them in rows 0..30)
    // (one opaque LDS address: left to itself hipcc keeps a register per distance through the row loop, which has none to spare)
    [[maybe_unused]] lds_u8 *rec = (lds_u8 *)s_mem + ((wave >> 2) * kRowB + (6 * (wave & 3) + 4) * 1024 + lane * 16 - kRecBack);
    if constexpr (kPairs) asm volatile("" : "+v"(rec));
    const long nbatch = (n + 16 * W - 1) / (16 * W);
    unsigned char *ring = s_mem + kRingO + wave * (kSlots * 2048);
    BatchWalk walk{(long)blockIdx.x, nbatch, (long)gridDim.x};
    [[maybe_unused]] RowSpan span{0, 32, 0, 32, 7, true};
    [[maybe_unused]] int role = 0, n_roles = 1;
    if constexpr (kKp) {
        if constexpr (kSplit) {
            // workgroup id -> (batch, role): ids 8 R k + 8 role + x serve batch 8 k + x -- the R workgroups of a batch sit 8 ids
            // apart (dispatch deals ids to the 8 XCDs round-robin: they share an L2, a matter of speed only) and the consumer
            // (role R - 1) has the highest id of its batch (its partners were dispatched before it)
            n_roles = ks.split;
            const long id = blockIdx.x, grp = id / (8 * n_roles), in = id - grp * (8 * n_roles);
            role = (int)(in >> 3);
            const long b = grp * 8 + (in & 7);
            walk = BatchWalk{b, b < nbatch ? b + 1 : b, 1};
            span = row_span(role, n_roles);
        } else {
            walk = kp_batches(nbatch);
        }
        if (walk.cur >= walk.end) return;
        // per-level geometry into LDS (lanes look up different levels: see LevelTable)
        int *lv = reinterpret_cast<int *>(s_mem + kRingO + W * kSlots * 2048);
        long *lv_off = reinterpret_cast<long *>(lv + 5 * kMaxPyrLevels);
        if (threadIdx.x < kMaxPyrLevels) {
            const int l = threadIdx.x;
            int w_ = 0, h_ = 0, pi_ = 0, ap_ = 0;
            long of_ = 0;
#pragma unroll
            for (int j = 0; j < kMaxPyrLevels; ++j)
                if (j == l) { w_ = ks.pd.w[j]; h_ = ks.pd.h[j]; pi_ = ks.pd.pitch[j]; ap_ = ks.pd.apron[j]; of_ = ks.pd.offset[j]; }
            lv[l] = w_; lv[kMaxPyrLevels + l] = h_; lv[2 * kMaxPyrLevels + l] = pi_; lv[3 * kMaxPyrLevels + l] = ap_;
            lv_off[l] = of_;
        }
        __syncthreads();
        const LevelTable lt{ks.pd.levels, lv, lv + kMaxPyrLevels, lv + 2 * kMaxPyrLevels, lv + 3 * kMaxPyrLevels};
        if (wave >= W) {
            if constexpr (kSplit) kp_produce_split<W>(ks, lt, lv_off, n, walk.cur, span, s_mem, lut_rows, wave - W, lane);
            else kp_produce<W>(ks, lt, lv_off, n, walk, s_mem, lut_rows, wave - W, lane);
            return;
        }

        if constexpr (ablate::kConsumerPrio >= 0) __builtin_amdgcn_s_setprio(ablate::kConsumerPrio);
    }
    // DMA writes are lane-linear (lane l -> bytes [16l, 16l+16) of a 1 KiB piece): lane (p, q) moves the 16-B
    // chunk q of its patch's half-row; the reader (p, q) needs chunk q of half 0 and its mirror, chunk 3 - q of half 1
    // (unfolded: chunks 2(q&1), 2(q&1)+1 of half q>>1, 256 bytes apart).
    const unsigned char *ring_lane = kFold ? ring + (q * 16 + p) * 16 : ring + (q >> 1) * 1024 + ((2 * (q & 1)) * 16 + p) * 16;
    [[maybe_unused]] const unsigned char *ring_mirror = ring + 1024 + ((3 - q) * 16 + p) * 16;

    long batch = walk.cur;
    if (batch >= walk.end) return;
    // Claim forms: the batch after the current one is HELD, one ahead -- `more` and `src_next` are known from a batch's first
    // instruction, as the ring prefetch of rows 27..30 and the epilogue's request for LUT row 0 need them -- and the one after
    // that is drawn during the current batch's row 0 (patch_row).  A ticket is one relaxed agent-scope atomic add by one lane
    // of wave 0 (request_ticket), without a fence: no data passes between workgroups, only the number.  Nobody waits for
    // anybody: a ticket at or beyond the launch's last batch (the count may be the device's, below the host's) ends the
    // workgroup.
    // The first ticket is drawn here, before any LDS-DMA request is in flight, and handed over by a barrier of its own.
    [[maybe_unused]] unsigned *claim_ctr = nullptr;
    [[maybe_unused]] long held = 0;           // claim forms: the batch after `batch`
    [[maybe_unused]] unsigned drawn = 0;      // ... and the ticket of the one after that, read from ticket_word in row 31
    if constexpr (kClaimForm) {
        claim_ctr = ks;
        held = batch + walk.step;
        if (claim_ctr) {
            if (wave == 0) {
                unsigned t = 0;
                request_ticket(claim_ctr, t);
                await_ticket(t);
                if (lane == 0) *ticket_word = t;
            }
            __syncthreads();
            held = (long)gridDim.x + __builtin_amdgcn_readfirstlane(*ticket_word);
            // (the word is next written at the end of row 0, behind that row's barrier, which no wave passes before this read
            //  has returned: __syncthreads waits for lgkmcnt(0))
        }
    }
    // the x-odd cartesian kernels' x-profile at the lane's folded pixels 4q .. 4q+3 (valu_odd_cart): loaded once, and landed
    // before the first LDS-DMA request -- the row loop itself issues no vector load (see wait_vmcnt)
    [[maybe_unused]] f32x2 oc_fx[2] = {pk_set(0.f), pk_set(0.f)};
    if constexpr (kOddV) {
        const f32x4 f = *reinterpret_cast<const f32x4 *>(odd_cart + 4 * q);
        oc_fx[0] = f32x2{f[0], f[1]};
        oc_fx[1] = f32x2{f[2], f[3]};
        asm volatile("" : "+v"(oc_fx[0]), "+v"(oc_fx[1]));
    }
    // lanes beyond the last patch recompute it: the wave's base is clamped the same way, so lane offsets stay >= 0
    auto raw_src = [&](const float *pt, long b) {
        const long b0 = b * (16 * W) + wave * 16;
        const long wave0 = b0 < n ? b0 : n - 1;                 // uniform
        const long pidx = b0 + p < n ? b0 + p : n - 1;
        return RawSrc{reinterpret_cast<const unsigned char *>(pt + wave0 * 1024), (unsigned)(pidx - wave0) * 4096u + 16u * q};
    };
    {
        if constexpr (!kKp) {
            const RawSrc src = raw_src(patches, batch);
            if constexpr (kPairs) {
#pragma unroll
                for (int r = 0; r < kRingSlots; ++r) issue_raw_row(src, r, ring, r);
            } else {
#pragma unroll
                for (int r = -2; r <= 3; ++r) issue_raw_row(src, clamp_row(r), ring, r + 2);
            }
        }
        issue_lut_row<W, kFold, kOddV>(lut_rows, kSplit ? span.lo : 0, s_mem, wave, lane);
    }
    int slot0 = 0;   // keypoint mode: ring slot of raw row 0 of the current batch
    unsigned par = 0;  // LUT row buffer holding the row about to be consumed
    ablate::PhaseClock phase;   // (instrument builds only: tools/phase_timing.py)
    phase.start();

    for (; batch < walk.end;) {
        // Launder the (uniform) table and buffer pointers once per batch.  Otherwise hipcc hoists one 64-bit per-lane VGPR
        // address per DMA / fragment load / store out of the batch loop and spills them (1.4 KB per lane for the
        // whitening fragments alone).  Spills matter beyond their cost here: scratch loads and stores count on vmcnt
        // like the LDS-DMA requests, stores retire out of order with respect to loads, and the f16 epilogue waits for its
        // DMA steps with COUNTED waits (wait_vmcnt<kDma>) -- a scratch store in flight there would let a wait pass
        // before its DMA has landed.  The Makefile fails the build if an f16 instantiation of this kernel uses scratch.
        const unsigned char *wf = wfrag, *lr = lut_rows;
        const float *bs = bias, *pt = patches;
        float *o = out, *ro = raw_out;
        const short *cm = colmap;
        asm volatile("" : "+s"(wf), "+s"(bs), "+s"(lr), "+s"(o), "+s"(ro), "+s"(cm), "+s"(pt));
        const float *oc_tab = odd_cart;
        const long base = batch * (16 * W) + wave * 16;
        const long next_batch = kClaimForm ? held : batch + walk.step;
        const bool more = next_batch < walk.end;
        // (keypoint mode: pt is null and these stay unused)
        const RawSrc src = kKp ? RawSrc{nullptr, 0u} : raw_src(pt, batch);
        const RawSrc src_next = !kKp && more ? raw_src(pt, next_batch) : src;

        f32x4 acc[kNAcc];
#pragma unroll
        for (int t = 0; t < kNAcc; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // valu_odd_cart: the batch's sums for the x-odd cartesian columns -- [m | sin_o, -cos_o of k = 1..3][gy_b]
        [[maybe_unused]] float oc[kOddCartSums][3];
#pragma unroll
        for (int s = 0; s < kOddCartSums; ++s)
#pragma unroll
            for (int b = 0; b < 3; ++b) oc[s][b] = 0.f;
        // blurred rows g and g-1 (row -1 replicates row 0) in the lane's pixel order, and row g just outside the lane's
        // pixels: folded (blur_row_fold_impl) x = 4q-1, 4q+4, 27-4q, 32-4q; unfolded x = 8q-1, 8q+8
        float cur[8], prv[8], cur_nb[4] = {0.f, 0.f, 0.f, 0.f};
        // patch mode: the vertical sums of hb(g+2), carried from the first body of a row pair (g, g+1) to its second
        [[maybe_unused]] float vnext[8];
        [[maybe_unused]] Halo hnext;
        [[maybe_unused]] bool last_six = false;          // pair forms: the middle-row loop is on rows 25..30
        [[maybe_unused]] int s0 = 1;                     // one-row patch forms: ring slot of raw row g-1 (rows g-1..g+3 feed hb(g+1))

        // The first and the last row of a batch differ from the 30 between them (two blurs / no blur): they are separate
        // copies of the row body, so that the loop over the middle rows carries none of their branches -- hipcc speculated
        // the last row's "row 32 = row 31" copy into every row (ten v_mov).
        //
        // The pair forms (kPairs: patch mode, f16x3) walk the middle rows in PAIRS (g, g+1), g odd.  Raw row r of the batch
        // lives in ring slot r mod 6 -- a compile-time slot in every body, because the middle-row loop is unrolled over three
        // pairs (six rows) -- and the six slots hold exactly raw rows g-1 .. g+4, which hb(g+1) (rows g-1 .. g+3) and hb(g+2)
        // (rows g .. g+4) need between them.  The pair's first body reads each slot ONCE (6 ring reads per row instead of
        // 10), runs both vertical passes and the horizontal pass of hb(g+1); its second body runs the horizontal pass of
        // hb(g+2) and touches the ring not at all.  Once read, the slots of rows g-1 and g take rows g+5 and g+6.  Rows beyond
        // the patch are never fetched: the taps of hb(0), hb(1), hb(30) and hb(31) that fall outside read the slot of row 0 or
        // row 31 (compile-time maps of row 0's body and of the last pair's).
        // The next batch's rows 0..5 go into their own slots as those fall free: 2 and 3 in pair (27, 28), the rest in pair
        // (29, 30).  pos = -1: a body of its own (rows 0 and 31; every row of the one-row forms); 2 P + s: body s of pair P of
        // the three.
        auto patch_row = [&](auto kind, const int g, auto pos) __attribute__((always_inline)) {
            constexpr bool kFirst = decltype(kind)::value == 0, kLast = decltype(kind)::value == 2;
            constexpr bool kFirstInner = decltype(kind)::value == 3;   // row-split form: a first row that is not row 0
            constexpr int kPos = decltype(pos)::value;
            constexpr bool kPairFirst = kPos >= 0 && (kPos & 1) == 0, kPairSecond = kPos >= 0 && (kPos & 1) == 1;
            constexpr int kSlot0 = kPos >= 0 ? (kPos & ~1) : 0;   // ring slot of raw row g-1 in a pair's first body
            static_assert(kPairs ? (kFirst || kLast) == (kPos < 0) : kPos < 0, "the pair forms' rows 1..30 go in pairs");
            constexpr bool kRowDma = !ablate::kNoRowDma;   // (LF_ABLATE_ROW_DMA: the row loop's requests are formed, not issued)

            // LUT row g and the ring rows the body reads have landed (own DMA: vmcnt; everyone's: barrier); row g-1 is done
            phase.mark(7);
            if constexpr (!ablate::kNoRowSync) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            phase.mark(0);
            // Claim forms.  Row 31: the ticket wave 0 left at the end of row 0 is read here, right behind the barrier, where the
            // wave has nothing in flight (an LDS read further down makes hipcc drain vmcnt first: it cannot tell the read from
            // the LDS its DMA requests write).  Row 0: lane 0 of wave 0 draws the ticket of the batch after the held one, if
            // the held one exists (request_ticket).  The returning atomic counts on vmcnt: it stands HERE because the next
            // wait of every wave is then a vmcnt(0) -- row 1's, and before it wave 0's own at the end of this row, which hands
            // the ticket over -- and 31 row barriers lie between it and the counted waits of finish_descriptors (wait_vmcnt),
            // where nothing but the epilogue's own requests may be in flight.
            [[maybe_unused]] unsigned ticket = 0;
            if constexpr (kClaimForm && kLast) drawn = __builtin_amdgcn_readfirstlane(*ticket_word);
            if constexpr (kClaimForm && kFirst)
                if (claim_ctr && more && wave == 0) request_ticket(claim_ctr, ticket);
            const unsigned char *brow = s_mem + par * kRowB + lane * 16;
            // row buffer par ^ 1 is free: next LUT row; during row 31 the f16 epilogue's first whitening step instead
            // (keypoint mode: the producer waves request LUT rows 1..31 -- an LDS-DMA request stalls its issuer for 60-180
            // cycles, which a producer can afford -- so a describe wave issues no memory instruction in the row loop)
            if (f16_family(POOL) ? !kLast : (!kLast || more)) {
                if constexpr (!kKp) issue_lut_row<W, kFold, kOddV, kRowDma>(lr, (g + 1) & 31, s_mem + (par ^ 1) * kRowB, wave, lane);
            } else if (f16_family(POOL)) {
                issue_w_step<W>(wf, 0, s_mem, wave, lane);
            }
            par ^= 1;
            constexpr int kMTiles = kOddV ? 2 : 3;   // m-stream fragments
            BFrag bm[kMTiles];
#pragma unroll
            for (int t = 0; t < kMTiles; ++t) bm[t] = load_b(brow, t);
            // gy_0..2 of row g for the x-odd cartesian columns: a wave-uniform address -- a scalar load, not a vector one
            [[maybe_unused]] f32x4 oc_gy = {0.f, 0.f, 0.f, 0.f};
            if constexpr (kOddV) oc_gy = *reinterpret_cast<const f32x4 *>(oc_tab + 16 + 4 * g);

            // One-row patch forms: raw row g+4 goes into the slot of row g-2, whose last reader was the blur of the previous
            // iteration: for g >= 1 it is requested here, a whole row before the vmcnt(0) that waits for it (counters: the
            // waves spend 29 % of their time in s_waitcnt and only 2 % of that on LDS), for g == 0 after the first blur below.
            if constexpr (!kKp && !kPairs)
                if (!kFirst && !kLast && g <= 29) issue_raw_row<kRowDma>(src, clamp_row(g + 4), ring, s0 == 0 ? kRingSlots - 1 : s0 - 1);
            float nxt[8], nxt_nb[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (!kPairs) {
                // keypoint mode: the five raw rows of hb(y) are rows y-2 .. y+2 clamped to the patch (replicate border), each
                // in its slot of the producer's ring
                auto kp_slot = [&](int y, int i) {
                    int r_ = y - 2 + i;
                    r_ = r_ < 0 ? 0 : (r_ > 31 ? 31 : r_);
                    return (slot0 + r_) % kRingSlotsKp;
                };
                // one blurred row, by either lane map; tap(i) = ring slot of the i-th of its five raw rows
                auto blur = [&](auto tap, float (&o)[8], float (&o_nb)[4]) __attribute__((always_inline)) {
                    if constexpr (kFold) blur_row_fold_impl(ring_lane, ring_mirror, tap, addr_l, addr_r, has_l, has_r, o, o_nb);
                    else blur_row_impl(ring_lane, tap, addr_l, addr_r, has_l, has_r, o, o_nb[0], o_nb[1]);
                };
                auto ring_tap = [](int first) {   // one-row patch forms: consecutive slots of the 6-slot ring from `first`
                    return [first](int i) { const int sl = first + i; return sl >= kRingSlots ? sl - kRingSlots : sl; };
                };
                if (kFirst) {  // first blurred row of the batch (one-row patch forms: rows -2..2 sit in slots 0..4)
                    if constexpr (kKp) blur([&](int i) { return kp_slot(0, i); }, cur, cur_nb);
                    else blur(ring_tap(0), cur, cur_nb);
#pragma unroll
                    for (int x = 0; x < 8; ++x) prv[x] = cur[x];
                }
                if constexpr (kFirstInner) {   // blurred rows g - 1 and g themselves: nothing replicates
                    float edge[4];
                    blur([&](int i) { return kp_slot(g - 1, i); }, prv, edge);
                    blur([&](int i) { return kp_slot(g, i); }, cur, cur_nb);
                }
                if (!kLast) {  // hb(g+1) from raw rows g-1..g+3 (one-row patch forms: slots s0..s0+4)
                    if constexpr (kKp) blur([&](int i) { return kp_slot(g + 1, i); }, nxt, nxt_nb);
                    else blur(ring_tap(s0), nxt, nxt_nb);
                }
            } else {
                const unsigned char *ring_b = kFold ? ring_mirror : ring_lane + 256;   // the lane's second block of a raw row
                auto hblur = [&](const float (&v)[8], float (&o)[8], float (&o_nb)[4]) __attribute__((always_inline)) {
                    if constexpr (kFold) hblur_row_fold_rec(v, halo_records(v, rec), rec, has_l, has_r, o, o_nb);
                    else hblur_row(v, addr_l, addr_r, has_l, has_r, o, o_nb[0], o_nb[1]);
                };
                auto slot = [](int j) { return (kSlot0 + j) % kRingSlots; };   // of the j-th raw row a body reads
                if constexpr (kFirst) {  // hb(0) from raw rows {0, 0, 0, 1, 2}, hb(1) from {0, 0, 1, 2, 3}: slots 0..3
                    float v0[8];
                    vblur_pair<4>(ring_lane, ring_b, slot, [](int i) { return i < 2 ? 0 : i - 2; },
                                  [](int i) { return i < 1 ? 0 : i - 1; }, v0, vnext);
                    hblur(v0, cur, cur_nb);
#pragma unroll
                    for (int x = 0; x < 8; ++x) prv[x] = cur[x];
                    hblur(vnext, nxt, nxt_nb);
                } else if constexpr (kPairFirst) {
                    float v1[8];
                    if (kPos == 4 && last_six)   // pair (29, 30): raw rows 28..31, row 31 standing in for rows 32 and 33
                        vblur_pair<4>(ring_lane, ring_b, slot, [](int i) { return i < 3 ? i : 3; },
                                      [](int i) { return i < 2 ? i + 1 : 3; }, v1, vnext);
                    else                         // raw rows g-1 .. g+4
                        vblur_pair<6>(ring_lane, ring_b, slot, [](int i) { return i; }, [](int i) { return i + 1; }, v1, vnext);
                    // The slots of raw rows g-1 and g are free once read: they take rows g+5 and g+6, requested here, nearly a
                    // whole row before the vmcnt(0) at the top of the pair's second body.  (The second body reads no ring
                    // row and could let them fly on behind a counted wait for its LUT row alone -- but hipcc puts a vmcnt(0)
                    // of its own before that body's LDS reads, which it cannot tell from the LDS these requests write.)
                    // The last two pairs request the next batch's first rows instead, into their own slots.
                    // The wait makes "once read" an ordering: the ring reads above have returned before a request can write.
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (!last_six || kPos == 0) {            // (rows 30 and 31 are the last of the batch)
                        issue_raw_row<kRowDma>(src, g + 5, ring, kSlot0);
                        issue_raw_row<kRowDma>(src, g + 6, ring, kSlot0 + 1);
                    } else if (more) {
                        if constexpr (kPos == 2) {
                            issue_raw_row<kRowDma>(src_next, 2, ring, 2);
                            issue_raw_row<kRowDma>(src_next, 3, ring, 3);
                        } else {
#pragma unroll
                            for (int r = 0; r < kRingSlots; ++r)
                                if (r != 2 && r != 3) issue_raw_row<kRowDma>(src_next, r, ring, r);
                        }
                    }
                    // both rows' halos now, behind the requests (the second body then starts on its filter at once and
                    // the area is free for its edge pixels): hb(g+2)'s four pairs wait with its vertical sums
                    const Halo h1 = halo_records(v1, rec);
                    hnext = halo_records(vnext, rec);
                    hblur_row_fold_rec(v1, h1, rec, has_l, has_r, nxt, nxt_nb);
                } else if constexpr (kPairSecond) {
                    hblur_row_fold_rec(vnext, hnext, rec, has_l, has_r, nxt, nxt_nb);
                }
            }
            if (kLast) {  // row 32 replicates row 31
#pragma unroll
                for (int x = 0; x < 8; ++x) nxt[x] = cur[x];
#pragma unroll
                for (int x = 0; x < 4; ++x) nxt_nb[x] = cur_nb[x];
            }
            // one-row patch forms: the slot of raw row g-2 is free now (its last reader was the blur above when g == 0)
            asm volatile("" ::: "memory");
            if constexpr (!kKp && !kPairs) {
                if (kFirst) {
                    issue_raw_row<kRowDma>(src, g + 4, ring, s0 == 0 ? kRingSlots - 1 : s0 - 1);
                } else if (kLast && more) {
#pragma unroll
                    for (int r = -2; r <= 3; ++r) issue_raw_row<kRowDma>(src_next, clamp_row(r), ring, r + 2);  // next batch's first rows
                }
                s0 = s0 == kRingSlots - 1 ? 0 : s0 + 1;
            }
            phase.mark(1);

            f32x2 m[4], c1[4], s1[4];
            {
                f32x2 gx[4], gy[4], r2n[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // patch_gradients.glsl:94-100, two pixels at a time
                    const int x = 2 * e;
                    f32x2 left, right;
                    if constexpr (kFold) {   // cur[0..3] ascending in x, cur[4..7] descending (blur_row_fold_impl)
                        left = e == 0 ? f32x2{cur_nb[0], cur[0]} : e == 1 ? f32x2{cur[1], cur[2]}
                               : e == 2 ? f32x2{cur[5], cur[6]} : f32x2{cur[7], cur_nb[2]};
                        right = e == 0 ? f32x2{cur[1], cur[2]} : e == 1 ? f32x2{cur[3], cur_nb[1]}
                                : e == 2 ? f32x2{cur_nb[3], cur[4]} : f32x2{cur[5], cur[6]};
                    } else {
                        left = f32x2{x == 0 ? cur_nb[0] : cur[x - 1], cur[x]};
                        right = f32x2{cur[x + 1], x == 6 ? cur_nb[1] : cur[x + 2]};
                    }
                    // left - right, plus +0.0: the value unchanged, but -0.0 (a blurred -0.0 on the left of a +0.0 -- the blur of
                    // negative denormals underflows to it, fma or not) becomes +0.0, so that the sign bit gradient_direction
                    // takes from gx is never the sign of a zero: the shader's (cos, sin) = (1, 0) at gx == -0.0, atan2.glsl:29-45
                    // (pair forms: left and right straddle the register pairs cur lives in, and a packed subtraction wants each of
                    //  them in an aligned pair of its own -- ten moves a row; two single subtractions need none and write the pair
                    //  the packed + 0.0 then takes.  Per lane the same two IEEE operations.)
                    if constexpr (kPairs) gx[e] = f32x2{left.x - right.x, left.y - right.y} + pk_set(0.0f);
                    else gx[e] = (left - right) + pk_set(0.0f);
                    gy[e] = f32x2{nxt[x], nxt[x + 1]} - f32x2{prv[x], prv[x + 1]};      // down - up
                    r2n[e] = pk_fma(gy[e], gy[e], gx[e] * gx[e]);
                    const f32x2 r2 = r2n[e] + pk_set(1e-8f);
                    m[e] = f32x2{__builtin_amdgcn_sqrtf(__builtin_amdgcn_sqrtf(r2.x)),
                                 __builtin_amdgcn_sqrtf(__builtin_amdgcn_sqrtf(r2.y))};
                }
                if constexpr (ablate::kNoFrontEnd) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { c1[e] = gx[e]; s1[e] = gy[e]; }
                } else {
                    gradient_direction4<ANGLE>(gx, gy, r2n, c1, s1);
                }
            }
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                prv[x] = cur[x];
                cur[x] = nxt[x];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) cur_nb[x] = nxt_nb[x];
            phase.mark(2);

            // m stream x (polar | cartesian) kernels: accumulator tiles 0-2
            BFrag gfrag = load_b(brow, 3);   // first harmonic: P0
            {
                AFrag<kMPool> am;
                if constexpr (kFold) {   // [m_e | m_o]
                    f32x2 mf[4];
                    fold_sum(m, mf[0], mf[1]);
                    fold_diff(m, mf[2], mf[3]);
                    if constexpr (kOddV) odd_cart_row(oc_fx, oc_gy, mf[2], mf[3], oc[0]);
                    am.set(mf);
                } else {
                    am.set(m);
                }
#pragma unroll
                for (int t = 0; t < kMTiles; ++t) mma_part<kMPool, 0>(am, bm[t], acc[t]);
#pragma unroll
                for (int t = 0; t < kMTiles; ++t) mma_part<kMPool, 1>(am, bm[t], acc[t]);
#pragma unroll
                for (int t = 0; t < kMTiles; ++t) mma_part<kMPool, 2>(am, bm[t], acc[t]);
            }
            phase.mark(3);
            // cos / sin streams of the three harmonics x their LUT tiles: accumulator tiles 3-20 (unfolded: 3-23)
            if constexpr (POOL == LF_POOL_F16_FP6) pool_harmonics_fp6(m, c1, s1, brow, gfrag, acc);
            else pool_harmonics<POOL>(m, c1, s1, brow, gfrag, acc, oc_fx, oc_gy, oc);
            phase.mark(4);
            // (patch mode: the row's share of the 21 sums is added HERE -- left alone, hipcc sinks the six rows' additions to
            //  the end of the unrolled loop body and spills their operands on the way)
            if constexpr (kPairs)
#pragma unroll
                for (int s = 0; s < kOddCartSums; ++s) asm volatile("" : "+v"(oc[s][0]), "+v"(oc[s][1]), "+v"(oc[s][2]));
            // claim forms, end of row 0: the ticket has had the row to return; row 1's barrier shows the word to every wave
            if constexpr (kClaimForm && kFirst) {
                if (claim_ctr && wave == 0) {
                    await_ticket(ticket);
                    if (lane == 0) *ticket_word = ticket;
                }
            }
            phase.mark(5);
        };
        constexpr std::integral_constant<int, -1> kOwnBody{};
        if constexpr (kSplit) {
            if (span.lo == 0) patch_row(std::integral_constant<int, 0>(), 0, kOwnBody);
            else patch_row(std::integral_constant<int, 3>(), span.lo, kOwnBody);
#pragma unroll 1
            for (int g = span.lo + 1; g < span.hi - 1; ++g) patch_row(std::integral_constant<int, 1>(), g, kOwnBody);
            if (span.consumer) patch_row(std::integral_constant<int, 2>(), span.hi - 1, kOwnBody);
            else patch_row(std::integral_constant<int, 1>(), span.hi - 1, kOwnBody);
            // (before the partial sums are published: sums over row subsets add, and the exchange keeps its 21 tiles)
            if constexpr (kOddV) rebuild_odd_cart(oc, lane, acc);
            // the partial sums meet: [batch][role][wave][tile][lane] f32x4, one counter per (batch, wave)
            unsigned *cnt = ks.xchg_cnt + batch * W + wave;
            // Every access to the exchange buffer and its counters is a relaxed atomic of agent scope: such a store is
            // complete (vmcnt) once it has reached the level of the memory system all XCDs see, such a load is served from
            // there -- no release / acquire fence, whose cost on this chip is a write-back and an invalidation of the whole L2
            // (the LUT rows and the pyramid every other workgroup is reading: measured, profiles/r06_row_split.md).
            typedef unsigned long long u64;
            if (!span.consumer) {
                u64 *dst = reinterpret_cast<u64 *>(ks.xchg + ((((long)batch * (n_roles - 1) + role) * W + wave) * kAccTiles) * 256) + lane;
#pragma unroll
                for (int t = 0; t < kAccTiles; ++t) {
                    const u64 v0 = ((u64)__float_as_uint(acc[t][1]) << 32) | __float_as_uint(acc[t][0]);
                    const u64 v1 = ((u64)__float_as_uint(acc[t][3]) << 32) | __float_as_uint(acc[t][2]);
                    __hip_atomic_store(dst + t * 128, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(dst + t * 128 + 64, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the wave's partial sums are where everyone sees them ...
                if (lane == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... before it counts itself in
                if (clk && blockIdx.x == 0 && threadIdx.x == 0) {
                    clk[2] = __builtin_readcyclecounter();
                    clk[3] = __builtin_amdgcn_s_memrealtime();
                }
                return;
            }
            int polls = 0;
            while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (unsigned)(n_roles - 1) &&
                   polls < kSplitSpinMax) {
                __builtin_amdgcn_s_sleep(1);
                ++polls;
            }
            asm volatile("" ::: "memory");
            if (polls >= kSplitSpinMax && lane == 0) atomicAdd(ks.xchg_cnt - 1, 1u);   // the error word: a partner never arrived
#pragma unroll 1
            for (int r = 0; r + 1 < n_roles; ++r) {
                const u64 *srcp = reinterpret_cast<const u64 *>(ks.xchg + ((((long)batch * (n_roles - 1) + r) * W + wave) * kAccTiles) * 256) + lane;
                // a partner's 21 tiles are requested in one go (42 loads in flight: one trip to memory per partner, not per
                // tile -- a workgroup of this form has a SIMD's 512 registers per wave) and added in tile order
                u64 v[2 * kAccTiles];
#pragma unroll
                for (int t = 0; t < 2 * kAccTiles; ++t)
                    v[t] = __hip_atomic_load(srcp + t * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < kAccTiles; ++t)
                    acc[t] += f32x4{__uint_as_float((unsigned)v[2 * t]), __uint_as_float((unsigned)(v[2 * t] >> 32)),
                                    __uint_as_float((unsigned)v[2 * t + 1]), __uint_as_float((unsigned)(v[2 * t + 1] >> 32))};
            }
            if (lane == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            // (the epilogue counts its own LDS-DMA requests on vmcnt: nothing of the above may still be in flight)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            patch_row(std::integral_constant<int, 0>(), 0, kOwnBody);
            if constexpr (!kPairs) {
#pragma unroll 1
                for (int g = 1; g < ablate::kRows - 1; ++g) patch_row(std::integral_constant<int, 1>(), g, kOwnBody);
                patch_row(std::integral_constant<int, 2>(), ablate::kRows - 1, kOwnBody);
            } else {   // five times three row pairs
                static_assert(ablate::kRows == 32, "LF_ABLATE_ROWS: the pair forms walk whole patches only");
#pragma unroll 1
                for (int g = 1; g < 31; g += 6) {
                    last_six = g == 25;
                    patch_row(std::integral_constant<int, 1>(), g, std::integral_constant<int, 0>());
                    patch_row(std::integral_constant<int, 1>(), g + 1, std::integral_constant<int, 1>());
                    patch_row(std::integral_constant<int, 1>(), g + 2, std::integral_constant<int, 2>());
                    patch_row(std::integral_constant<int, 1>(), g + 3, std::integral_constant<int, 3>());
                    patch_row(std::integral_constant<int, 1>(), g + 4, std::integral_constant<int, 4>());
                    patch_row(std::integral_constant<int, 1>(), g + 5, std::integral_constant<int, 5>());
                }
                patch_row(std::integral_constant<int, 2>(), 31, kOwnBody);
            }
            if constexpr (kOddV) rebuild_odd_cart(oc, lane, acc);
        }
        if constexpr (ablate::kNoEpilogue) {
            f32x4 sum = acc[0];
            for (int t = 1; t < kNAcc; ++t) sum += acc[t];
            if (base + p < n) *reinterpret_cast<f32x4 *>(out + (base + p) * 128 + 4 * q) = sum;
            if (f16_family(POOL)) {
                __syncthreads();
                if (more) issue_lut_row<W, kFold, kOddV>(lr, 0, s_mem, wave, lane);
            }
        } else {
            // (pair forms: whatever the epilogue derives from the lane's number alone is derived here, once per batch -- hoisted
            //  out of the batch loop it is seven registers held through a row loop that has none to spare)
            int lane_e = lane;
            if constexpr (kPairs) asm volatile("" : "+v"(lane_e));
            const long patch_e = base + (lane_e & 15);
            finish_descriptors<POOL, W>(acc, lane_e, wave, patch_e < n, patch_e, cm, wf, bs, o, ro, s_mem, lr, more);
        }
        phase.mark(6);
        if constexpr (kKp) slot0 = (slot0 + 8) % kRingSlotsKp;
        wg_clock.batch_done();
        batch = next_batch;
        if constexpr (kClaimForm) held = claim_ctr ? (long)gridDim.x + drawn : batch + walk.step;
    }
    phase.dump(out, wave, lane);
    if constexpr (!kKp) wg_clock.leave(out, n_host);
    if (clk && blockIdx.x == 0 && threadIdx.x == 0) {
        clk[2] = __builtin_readcyclecounter();
        clk[3] = __builtin_amdgcn_s_memrealtime();
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// This source is compiled twice (Makefile): as is -- the patch-mode launcher, scheduled with max-ILP -- and with
// -DLF_DESCRIBE_KP -- the keypoint-mode launcher alone, under hipcc's default scheduling strategy: with max-ILP the two exact
// angle modes of the keypoint kernel need 259 registers (three spilled, which the counted vmcnt waits of the epilogue
// forbid), with the default strategy 203-209.
#ifndef LF_DESCRIBE_KP
// n_dev != nullptr: the patch count is read on the device (<= n, which then only sizes the grid)
void launch_describe(const float *patches, long n, const unsigned long long *n_dev, const DeviceConsts &dc,
                     int angle_mode, int pool_mode, float *out, float *raw_out, int num_cus, hipStream_t stream, int waves,
                     unsigned long long *clk, unsigned *claim) {
    if (n <= 0) return;
    // one 100-152 KiB-LDS workgroup per CU; requests of at most one round of 64-patch workgroups take the 4-wave form
    const bool small = ablate::kForceFourWaves || waves == 4 || (waves != 8 && n <= 64L * num_cus);
    const long nbatch = small ? (n + 63) / 64 : (n + 127) / 128;
    const unsigned grid = (unsigned)(nbatch < num_cus ? nbatch : num_cus);
    // Batches are claimed at run time where a workgroup has at least kClaimRounds WHOLE batches to walk: whole CUs and XCDs
    // run a few per cent apart, and dealt statically the slowest one ends the launch (NOTEBOOK.md, the claims section).  A
    // shorter launch keeps the static walk: its tail is a round of batches whatever the dealing.  The counter is cleared on
    // the launch stream just before the launch, so a captured launch carries its memset with it; with n_dev the host's n only
    // bounds the tickets that can be valid.
    if (small || !claim || !f16_family(pool_mode) || n / 128 < kClaimRounds * grid) claim = nullptr;
    if (claim && hipMemsetAsync(claim, 0, sizeof(unsigned), stream) != hipSuccess) return;   // (the caller reads the last error)
    const bool f16 = f16_family(pool_mode);
    const unsigned char *lut = pool_mode == LF_POOL_F16_FP6 ? reinterpret_cast<const unsigned char *>(dc.pool_b_fp6)
                               : f16                        ? reinterpret_cast<const unsigned char *>(dc.pool_b_f16)
                                                            : reinterpret_cast<const unsigned char *>(dc.pool_b_f32);
    const bool unfolded = !fold_form(pool_mode);   // LF_POOL_F16_FP6: its own packed order and whitening fragments
    const unsigned char *wf = unfolded ? reinterpret_cast<const unsigned char *>(dc.white_a_f16_unfolded)
                              : f16    ? reinterpret_cast<const unsigned char *>(dc.white_a_f16)
                                       : reinterpret_cast<const unsigned char *>(dc.white_a_f32);
    const short *colmap = unfolded ? dc.colmap_unfolded : dc.colmap;
#define LF_LAUNCH_W(A, P, WV)                                                                                          \
    hipLaunchKernelGGL((mkd_pool<A, P, WV, kSrcPatches>), dim3(grid), dim3(64 * WV), 0, stream, patches, n, n_dev, lut, \
                       colmap, wf, dc.white_bias, dc.odd_cart, out, raw_out, WV == 8 ? claim : (unsigned *)nullptr, clk)
#define LF_LAUNCH(A, P)            \
    do {                           \
        if (small) LF_LAUNCH_W(A, P, 4); \
        else LF_LAUNCH_W(A, P, 8); \
    } while (0)
    if (pool_mode == LF_POOL_F16_FP6) {
        if (angle_mode == LF_ANGLE_EXACT) LF_LAUNCH(LF_ANGLE_EXACT, LF_POOL_F16_FP6);
        else if (angle_mode == LF_ANGLE_EXACT_ZERO) LF_LAUNCH(LF_ANGLE_EXACT_ZERO, LF_POOL_F16_FP6);
        else LF_LAUNCH(LF_ANGLE_SHADER, LF_POOL_F16_FP6);
    } else if (f16) {
        if (angle_mode == LF_ANGLE_EXACT) LF_LAUNCH(LF_ANGLE_EXACT, LF_POOL_F16X3);
        else if (angle_mode == LF_ANGLE_EXACT_ZERO) LF_LAUNCH(LF_ANGLE_EXACT_ZERO, LF_POOL_F16X3);
        else LF_LAUNCH(LF_ANGLE_SHADER, LF_POOL_F16X3);
    } else {
        if (angle_mode == LF_ANGLE_EXACT) LF_LAUNCH(LF_ANGLE_EXACT, LF_POOL_F32);
        else if (angle_mode == LF_ANGLE_EXACT_ZERO) LF_LAUNCH(LF_ANGLE_EXACT_ZERO, LF_POOL_F32);
        else LF_LAUNCH(LF_ANGLE_SHADER, LF_POOL_F32);
    }
#undef LF_LAUNCH_W
#undef LF_LAUNCH
}

#else   // LF_DESCRIBE_KP
// Keypoint mode in one launch: 4 describe waves + 4 producer waves per workgroup, 64 keypoints per batch, one workgroup
// per CU (144 KiB of LDS), persistent; requests of at most 8192 keypoints: 2 + 2 waves, 32 keypoints per workgroup (below).
static long nbatch32(long n) { return (n + 31) / 32; }
size_t kp_split_exchange_bytes(int num_cus) {
    // R = 4: num_cus / 4 batches x 3 partial roles; R = 2: num_cus / 2 x 1 -- the larger of the two, x 2 waves x 21 tiles x 1 KiB
    return size_t(num_cus / 4 + 8) * 3 * 2 * kAccTiles * 1024;
}
size_t kp_split_counter_words(int num_cus) { return 1 + size_t(num_cus / 2 + 8) * 2; }   // the error word, then [batch][wave]

void launch_describe_keypoints(const float *pyr, long pyr_stride, const PyramidDesc &pd, const float *kps,
                               const unsigned *frame_of_kp, unsigned n_frames, long n, const unsigned long long *n_dev,
                               float psf, const DeviceConsts &dc, int angle_mode, float *out, int num_cus, hipStream_t stream,
                               unsigned long long *clk, float *xchg, unsigned *xchg_words, long form_n) {
    if (n <= 0) return;
    if (form_n < n) form_n = n;
    // A request of at most one round of 32-keypoint workgroups (<= 32 x CUs = 8192 keypoints: a frame at the reference's own
    // settings, top_n 2000 / max_features 3000) takes the 2 + 2-wave form: every wave has a SIMD to itself -- the describe
    // waves do not share theirs with a producer -- and the launch spreads over twice as many CUs.  It is a launch's latency
    // that this shortens; on full batches the 4 + 4 form's eight waves per CU are the faster arrangement.
    const bool narrow = n <= 32L * num_cus;      // (with n_dev, n is the capacity: the count on the device is no larger)
    const long per_wg = narrow ? 32 : 64;
    const long nbatch = (n + per_wg - 1) / per_wg;
    const unsigned grid = (unsigned)(nbatch < num_cus ? nbatch : num_cus);
    const unsigned char *lut = reinterpret_cast<const unsigned char *>(dc.pool_b_f16);
    const unsigned char *wf = reinterpret_cast<const unsigned char *>(dc.white_a_f16);
    KpSource ks;
    ks.pyr = pyr; ks.pyr_stride = pyr_stride; ks.kps = kps; ks.frame_of = frame_of_kp; ks.n_frames = n_frames ? n_frames : 1u;
    ks.psf = psf; ks.pd = pd;
    ks.split = 1; ks.xchg = nullptr; ks.xchg_cnt = nullptr;
    // The row-split form where R workgroups per batch of 32 are all resident at once (one per CU): R = 4 up to 8 x CUs
    // keypoints (2048), R = 2 up to 16 x CUs (4096) -- the reference's own operating point (top_n 2000, max_features 3000).
    // LF_MKD_KP_SPLIT=1 / 2 / 4 forces a form where it fits (tests, A/B runs).
    if (xchg && xchg_words) {
        // (the form follows form_n -- the capacity of the request the launch belongs to: lf_mkd_detect stage by stage, which
        //  knows its keypoint count, takes the form its recorded twin, which does not, takes for max_out: the same bits)
        const long nf8 = (nbatch32(form_n) + 7) / 8 * 8, nb8 = (nbatch32(n) + 7) / 8 * 8;
        int r = nf8 * 4 <= num_cus ? 4 : (nf8 * 2 <= num_cus ? 2 : 1);
        if (const char *e = getenv("LF_MKD_KP_SPLIT")) {
            const int want = atoi(e);
            if (want == 1 || ((want == 2 || want == 4) && nf8 * want <= num_cus)) r = want;
        }
        if (r > 1) {
            ks.split = r; ks.xchg = xchg; ks.xchg_cnt = xchg_words + 1;
            const unsigned sgrid = (unsigned)(nb8 * r);
#define LF_LAUNCH_KP_SPLIT(A)                                                                                                  \
    hipLaunchKernelGGL((mkd_pool<A, LF_POOL_F16X3, 2, kSrcKeypointsSplit>), dim3(sgrid), dim3(256), 0, stream,                    \
                       (const float *)nullptr, n, n_dev, lut, dc.colmap, wf, dc.white_bias, dc.odd_cart, out, (float *)nullptr, ks, clk)
            if (angle_mode == LF_ANGLE_EXACT) LF_LAUNCH_KP_SPLIT(LF_ANGLE_EXACT);
            else if (angle_mode == LF_ANGLE_EXACT_ZERO) LF_LAUNCH_KP_SPLIT(LF_ANGLE_EXACT_ZERO);
            else LF_LAUNCH_KP_SPLIT(LF_ANGLE_SHADER);
#undef LF_LAUNCH_KP_SPLIT
            return;
        }
    }
#define LF_LAUNCH_KP_W(A, WV)                                                                                          \
    hipLaunchKernelGGL((mkd_pool<A, LF_POOL_F16X3, WV, kSrcKeypoints>), dim3(grid), dim3(128 * WV), 0, stream,          \
                       (const float *)nullptr, n, n_dev, lut, dc.colmap, wf, dc.white_bias, dc.odd_cart, out, (float *)nullptr, ks, clk)
#define LF_LAUNCH_KP(A)                 \
    do {                                \
        if (narrow) LF_LAUNCH_KP_W(A, 2); \
        else LF_LAUNCH_KP_W(A, 4);      \
    } while (0)
    if (angle_mode == LF_ANGLE_EXACT) LF_LAUNCH_KP(LF_ANGLE_EXACT);
    else if (angle_mode == LF_ANGLE_EXACT_ZERO) LF_LAUNCH_KP(LF_ANGLE_EXACT_ZERO);
    else LF_LAUNCH_KP(LF_ANGLE_SHADER);
#undef LF_LAUNCH_KP_W
#undef LF_LAUNCH_KP
}
#endif  // LF_DESCRIBE_KP

}  // namespace lfmkd
