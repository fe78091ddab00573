// Device helpers of the RANSAC verifiers' kernels (mkd_verify.hip: verify_prepare, ransac_score, ransac_select), whatever
// the model.  Everything here is a fixed sequence of IEEE operations under contraction OFF.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_verify_host.h"   // kInvalid, splitmix64, cholesky8: what a host compiler shares with the kernels

#pragma clang fp contract(off)

#include "mkd_scene.h"         // block_sum, under the contraction its copy here was compiled under

namespace lfmkd {
namespace {

constexpr int kThreads = kSumThreads;          // every verification kernel: 4 waves
constexpr int kWaves = kThreads / 64;
constexpr unsigned kMaxSlices = 16;            // row slices per (pair, hypothesis block) of a scoring launch

// rows [lo, hi) of a pair, as the offsets give them (a pair whose offsets decrease is empty)
__device__ __forceinline__ uint64_t pair_rows(const uint64_t *off, unsigned p, uint64_t &lo) {
    lo = off[p];
    const uint64_t hi = off[p + 1];
    return hi > lo ? hi - lo : 0;
}

struct Pt {
    float ax, ay, bx, by;
};

// row r of a pair: considered if its match indexes the pair's b rows; then its two points
__device__ __forceinline__ bool load_row(const float *ka, const float *kb, const int *match, uint64_t r, uint64_t nb, Pt &q) {
    const int m = match[r];
    if (m < 0 || uint64_t(m) >= nb) return false;
    q.ax = ka[5 * r];
    q.ay = ka[5 * r + 1];
    q.bx = kb[5 * uint64_t(m)];
    q.by = kb[5 * uint64_t(m) + 1];
    return true;
}

// (the workgroup sums are mkd_scene.h's block_sum: the butterfly within a wave, then the waves in order)

}  // namespace
}  // namespace lfmkd
