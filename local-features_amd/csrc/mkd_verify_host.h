// The pieces of the two RANSAC verifiers that a plain C++ compiler can read as well as hipcc: the sampler's hash and the
// refit's Cholesky solve (the per-pair record is mkd_verify_pair.h).  mkd_verify_common.h includes it for the device build
// and the two models' math headers (mkd_homography_math.h, mkd_fundamental_math.h) for both, so that a host program
// (tests/cpp/fundamental_twin.cpp, tests/cpp/guided_twin.cpp) is built from the very code
// the kernels run; mkd_device.h must not: the pragma below holds for the rest of any file that includes this one.  Only
// <math.h> / <stdint.h> are needed.  Everything here is a fixed sequence of IEEE operations under contraction OFF (a host
// build passes -ffp-contract=off as well: the pragma is clang's).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkd_verify_pair.h"   // VerifyPair, and the HIP qualifiers defined away without hipcc

#pragma clang fp contract(off)

namespace lfmkd {

namespace {

constexpr unsigned kInvalid = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Solves N x = r in place (x returned in r) for a symmetric 8x8 N by Cholesky; false if a pivot is at or below 1e-12 of N's
// largest diagonal element (or that element is not positive).  Every loop has constant bounds: the matrix stays in registers.
__host__ __device__ __forceinline__ bool cholesky8(double (&N)[8][8], double (&r)[8]) {
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) dmax = fmax(dmax, N[i][i]);
    const double floor = 1e-12 * dmax;
    bool ok = dmax > 0.0;
    // N = L L^T in the upper triangle read as L^T (row i of L^T = column i of L)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double d = N[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= N[k][j] * N[k][j];
        ok = ok && d > floor;
        const double l = sqrt(fmax(d, floor));
        N[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
            double s = N[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= N[k][j] * N[k][i];
            N[j][i] = s / l;
        }
    }
    // L y = r, then L^T x = y
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double s = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= N[k][i] * r[k];
        r[i] = s / N[i][i];
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double s = r[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) s -= N[i][k] * r[k];
        r[i] = s / N[i][i];
    }
    return ok;
}

}  // namespace
}  // namespace lfmkd
