// The per-pair normalisation record of the two RANSAC verifiers, and what lets a plain C++ compiler read the headers that
// share code with the kernels (mkd_verify_host.h, mkd_homography_math.h, mkd_fundamental_math.h, mkd_guided_math.h): without hipcc the HIP function qualifiers mean
// nothing.  mkd_device.h includes this file, so it holds NO floating-point pragma: a file-scope contraction pragma in a header
// holds for the rest of whatever includes it.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#endif

namespace lfmkd {

// RANSAC verification (mkd_verify.hip, both models): a pair's normalisation, written by verify_prepare
struct VerifyPair {
    float ca[2], sa;   // a: centroid, scale (RMS distance from the centroid becomes sqrt(2))
    float cb[2], sb;   // b: the same
    unsigned m, pad;   // considered matches
};

}  // namespace lfmkd
