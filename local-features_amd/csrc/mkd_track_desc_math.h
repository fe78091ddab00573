// The arithmetic of track descriptors (mkd_track_desc.hip; contract: include/lf_mkd.h, lf_mkd_track_descriptors_device): which
// observation contributes, which track is described, the centred sums from sums of raw bytes, the norm and the quantiser,
// every one __host__ __device__.  tests/cpp/track_desc_twin.cpp includes it under a plain C++ compiler (with
// -ffp-contract=off) and restates only the walk over a track, so the host twin is this code and no transcription of it.
// Needs <math.h> and <stdint.h> alone.  Every sum is an integer sum, exact in any order: with at most kTdMaxObs = 65 536
// contributors a sum of raw bytes is below 2^24, |S_k| below 2^23 and n2 = sum_k S_k^2 below 2^53, so int32, int64 and f64
// hold them alike.  The quantiser is three correctly rounded f64 operations (a product that is exact, sqrt, /) and rint, under
// contraction OFF.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_resect_math.h"   // rs_point_usable: the resection call's own rule for a track's point, one definition

#pragma clang fp contract(off)

namespace lfmkd {
namespace {

constexpr int kTdRow = 128;                      // bytes of a row
constexpr unsigned kTdMaxObs = 65536;            // positions of a track that are read: the first kTdMaxObs
constexpr int32_t kTdNoSpread = INT32_MIN;       // the spread of a zero row
constexpr unsigned kTdMaxState = 2;              // the largest min_state: the states triangulation and bundle adjustment write

// Position k of a track CONTRIBUTES iff it passes the state filter (no array: every state passes) and names a row of the pool.
__host__ __device__ __forceinline__ bool td_contributes(bool has_state, uint32_t state, uint32_t min_state, int32_t row,
                                                        uint64_t n_rows) {
    return (!has_state | (state >= min_state)) & (row >= 0) & (uint64_t(row) < n_rows);   // (no short circuit: no branch)
}
// A track is DESCRIBED iff there is no point array or its point passes resection's rule (finite X, Y, Z and w <= cmin).
__host__ __device__ __forceinline__ bool td_described(const float *points, uint64_t t, double cmin) {
    return points == nullptr || rs_point_usable(points + 4 * t, cmin);
}
// S_k = sum over the C contributors of (byte_k - 128), from the sum of their raw bytes
__host__ __device__ __forceinline__ int32_t td_centre(uint32_t byte_sum, uint32_t C) { return int32_t(byte_sum) - 128 * int32_t(C); }
__host__ __device__ __forceinline__ int64_t td_square(int32_t S) { return int64_t(S) * int64_t(S); }
__host__ __device__ __forceinline__ double td_norm(int64_t n2) { return sqrt(double(n2)); }
// q_k = clamp(rint(S_k scale / norm), -127, 127), ties to even (norm > 0; S_k scale is exact: 24 bits times 24 bits)
__host__ __device__ __forceinline__ int32_t td_quantize(int32_t S, double scale, double norm) {
    const double v = (double(S) * scale) / norm;
    const double r = rint(v);
    return r < -127.0 ? -127 : r > 127.0 ? 127 : int32_t(r);
}
// a contributor's term of its similarity with the track's row: (byte - 128) q
__host__ __device__ __forceinline__ int32_t td_term(uint32_t byte, int32_t q) { return (int32_t(byte) - 128) * q; }

}  // namespace
}  // namespace lfmkd
