// The table kernels' one workgroup-wide scan (mkd_track_table.hip, mkd_link_table.hip, mkd_select_edges.hip): each unit
// compiles its own copy, no device code crosses a translation unit.
#pragma once
#include <hip/hip_runtime.h>

namespace lfmkd {
namespace {

// Exclusive prefix sum over the workgroup's NT threads, in thread order, and the total.  s: 2 * NT elements of LDS.
template <typename T, int NT>
__device__ __forceinline__ T block_scan(T v, T *s, T &total) {
    const int t = threadIdx.x;
    int cur = 0;
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < NT; off <<= 1) {
        T x = s[cur * NT + t];
        if (t >= off) x += s[cur * NT + t - off];
        s[(cur ^ 1) * NT + t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const T incl = s[cur * NT + t];
    total = s[cur * NT + NT - 1];
    __syncthreads();                                          // s may be used again at once
    return incl - v;
}

}  // namespace
}  // namespace lfmkd
