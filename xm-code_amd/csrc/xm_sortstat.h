// xm_sortstat.h — workgroup helpers shared by the device queries that take order statistics (xm_pair.hip, xm_lift.hip): the bitonic sort of a
// power-of-two array in LDS or global memory, numpy's default percentile of its smallest values, and the integer sum over the workgroup.
// All of them are for workgroups of kSortThreads threads (four wavefronts) and are called by every thread of the workgroup.
// Include it BEHIND the translation unit's `#pragma clang fp contract(off)`: percentile() rounds every product and sum on its own only then.
#pragma once

#include <hip/hip_runtime.h>

#include "xm_stage.h"   // lane_id()

namespace xm {

constexpr int kSortThreads = kStageThreads;

__device__ inline double inf_() { return __longlong_as_double(0x7ff0000000000000ll); }

// sum over the workgroup, valid in every thread; ired: 4 ints
__device__ inline int block_sum_int(int v, int *ired) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if (lane_id() == 0) ired[threadIdx.x >> 6] = v;
    __syncthreads();
    return (ired[0] + ired[1]) + (ired[2] + ired[3]);
}
// ascending bitonic sort of S[0 .. KP), KP a power of two >= 2; ends with a barrier
template <class P>
__device__ inline void sort_values(P S, int KP) {
    for (int size = 2; size <= KP; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = (int)threadIdx.x; t < (KP >> 1); t += kSortThreads) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const auto x = S[i], y = S[j];
                if ((x > y) == up) { S[i] = y; S[j] = x; }
            }
            __syncthreads();
        }
}
// S[q] = f(q) for q < k, +inf behind; then sorted
template <class P, class F>
__device__ inline void fill_sort(P S, int KP, int k, F f) {
    for (int q = (int)threadIdx.x; q < KP; q += kSortThreads) S[q] = q < k ? f(q) : inf_();
    __syncthreads();
    sort_values(S, KP);
}
// numpy.percentile (linear) of the k smallest values of the sorted S at the fraction q (numpy's _lerp; the caller compiles with contraction off)
template <class P>
__device__ inline double percentile(P S, int k, double q) {
    const double pos = (double)(k - 1) * q;
    const double fl = floor(pos), t = pos - fl;
    const int i0 = (int)fl, i1 = i0 + 1 < k ? i0 + 1 : k - 1;
    const double a = S[i0], b = S[i1], d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

}  // namespace xm
