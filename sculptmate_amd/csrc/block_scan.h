// Wave and workgroup scans, ranks and sums of the count -> scan -> emit stages, and the ordered-float key of the atomic min / max.
// Device templates only: no kernels, no host state.
//
// Workgroups are one-dimensional, NWAVES * 64 threads, and EVERY thread of the workgroup calls (the functions hold a barrier).
// `s_w` is the caller's LDS array of NWAVES elements.  Barrier contract: a block_* function has exactly ONE barrier, between its
// writes of s_w and its reads, and none at its end -- a caller that uses the same s_w again (another call, a loop) puts its own
// __syncthreads() first.  block_scan_in_place closes every trip with that barrier itself, so s_w is free when it returns.
#pragma once
#include "common.h"

namespace sculpt {

// order-preserving map of fp32 onto uint32 (and back), so that integer atomics / comparisons give the float minimum and maximum
__host__ __device__ __forceinline__ unsigned f32_to_ordered(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ordered_to_f32(unsigned o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// inclusive prefix sum over the 64 lanes of the wave
template <typename T>
__device__ __forceinline__ T wave_inclusive_add(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// exclusive prefix sum of v over the workgroup in thread order; *total = the workgroup's sum, in every thread
template <int NWAVES, typename T>
__device__ __forceinline__ T block_exclusive_add(T v, T *s_w, T *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive_add(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const T s = s_w[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// one value per wave (the same in all its lanes) -> their sum, in every thread
template <int NWAVES, typename T>
__device__ __forceinline__ T block_sum_of_waves(T wave_value, T *s_w) {
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = wave_value;
    __syncthreads();
    T t = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) t += s_w[w];
    return t;
}

// sum of v over the workgroup, in every thread
template <int NWAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T *s_w) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return block_sum_of_waves<NWAVES>(v, s_w);
}

// number of set flags of the workgroup, in every thread
template <int NWAVES>
__device__ __forceinline__ unsigned block_flag_count(bool flag, unsigned *s_w) {
    return block_sum_of_waves<NWAVES>((unsigned)__popcll(__ballot(flag)), s_w);
}

// the flag's rank among the set flags of the workgroup (exclusive), in thread order
template <int NWAVES>
__device__ __forceinline__ unsigned block_flag_rank(bool flag, unsigned *s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_w[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned base = 0u;
    for (int w = 0; w < wave; ++w) base += s_w[w];   // < NWAVES trips
    return base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// exclusive scan of a[0..n) in place by ONE workgroup, ceil(n / (64 * NWAVES)) trips; returns the total to every thread.
// The carry needs no LDS word and no owner: every thread adds the same trip total to its own copy.
template <int NWAVES, typename T>
__device__ __forceinline__ T block_scan_in_place(T *__restrict__ a, int n, T *s_w) {
    T carry = 0;
    for (int base = 0; base < n; base += 64 * NWAVES) {
        const int i = base + threadIdx.x;
        const T v = i < n ? a[i] : T(0);
        T tot;
        const T ex = block_exclusive_add<NWAVES>(v, s_w, &tot);
        if (i < n) a[i] = carry + ex;
        carry += tot;
        __syncthreads();   // s_w is read: the next trip (or the caller) may write it
    }
    return carry;
}

}  // namespace sculpt
