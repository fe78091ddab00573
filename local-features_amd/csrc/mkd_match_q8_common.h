// The int8 matchers' small helpers and the batched form's workgroup shape, shared by mkd_match_q8.hip (match_q8_scan,
// match_q8_merge, match_q8_pairs), mkd_match_q8_edges.hip (match_q8_edges), mkd_match_q8_guided.hip (match_q8_guided_pairs),
// mkd_match_q8_knn.hip and mkd_match_q8_grouped.hip: each unit compiles its own copy, no device code crosses a translation
// unit.  The three batched kernels reach it through mkd_match_q8_batched.h, which holds their prologues and bodies.  The notes
// on the forms are in mkd_match_q8.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace lfmkd {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kQTileRows = 32;                     // rows of a / b per MFMA tile
constexpr int kQTileBytes = kQTileRows * 128;      // [chunk 8][row 32][16 B] = 4 KiB
constexpr int kSignBits = (int)0x80808080u;

__device__ __forceinline__ void q8_lds_dma16(const void *g, void *l) {
    __builtin_amdgcn_global_load_lds(g, reinterpret_cast<__attribute__((address_space(3))) void *>(
                                            reinterpret_cast<uintptr_t>(l)), 16, 0, 0);
}

// the same for one dword per lane
__device__ __forceinline__ void q8_lds_dma4(const void *g, void *l) {
    __builtin_amdgcn_global_load_lds(g, reinterpret_cast<__attribute__((address_space(3))) void *>(
                                            reinterpret_cast<uintptr_t>(l)), 4, 0, 0);
}

__device__ __forceinline__ int max3i(int a, int b, int c) { return max(max(a, b), c); }   // (v_max3_i32)

// the acceptance rule (lf_mkd.h): both conversions are exact (|sums| < 2^24, INT32_MIN = -2^31), one f32 multiplication
__device__ __forceinline__ int q8_decide(int best, int index, int second, float ratio) {
    return (index >= 0 && (ratio <= 0.f || (float)best * ratio > (float)second)) ? index : -1;
}

}  // namespace
}  // namespace lfmkd

// the batched forms' workgroup: kPWaves waves x kPTiles tiles of 32 rows of x, kPStage tiles of y per LDS stage
#ifndef LF_Q8_PAIRS_WAVES
#define LF_Q8_PAIRS_WAVES 4
#endif
#ifndef LF_Q8_PAIRS_TILES
#define LF_Q8_PAIRS_TILES 1
#endif
namespace lfmkd {
namespace {
constexpr int kPWaves = LF_Q8_PAIRS_WAVES, kPTiles = LF_Q8_PAIRS_TILES;   // 4 x 1 tile = 128 rows (measured beside 256 and 512)
constexpr int kPStage = 4;                                                // y tiles per LDS stage: 16 KiB
constexpr int kPThreads = 64 * kPWaves;
constexpr int kPRows = kPWaves * kPTiles * kQTileRows;
constexpr int kPPieces = kPStage * 256 / kPThreads;                       // 16-byte DMA pieces per thread and stage
static_assert(kPPieces * kPThreads == kPStage * 256 && (kPRows & (kPRows - 1)) == 0, "whole pieces, R a power of two");
}  // namespace
}  // namespace lfmkd
