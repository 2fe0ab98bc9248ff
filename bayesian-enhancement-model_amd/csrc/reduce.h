// Wave and workgroup reductions by shuffles (wave64), float or double.  The DPP reductions of the scans and of the x6 LayerNorm
// prologue are not these: they live with their kernels.  The library is built for wave64 only, hence the literal width.
#pragma once
#include <hip/hip_runtime.h>

// xor butterfly: every lane gets the result; lane 0 holds what a shuffle-down tree leaves there (the same pairs at every level).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// Sum over a workgroup of NW waves, returned to every thread: a shuffle-down tree leaves each wave's sum in its lane 0 (the value
// wave_sum gives every lane), the wave sums go through sh[NW] and are added left to right from zero.  The leading barrier lets a
// kernel reuse sh for its next sum.
template <int NW, typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    T s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += sh[w];
    return s;
}
