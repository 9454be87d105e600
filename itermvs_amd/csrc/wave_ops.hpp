// Wave64 and workgroup sums, scans and ranks, once: what the compaction kernels (fuse_points.hip, tsdf.hip) and the reductions of
// bn.hip, cloud_register.hip, colmap.hip and train_input.hip are built from.  Device only; shuffles and LDS, no atomics.  The
// workgroup forms expect blockDim.x = 64 * waves and are called by EVERY thread of the workgroup (they hold a barrier).
// wave_sum_all and wave_sum_lane0 add in different orders: for float and double the order is part of the result, so a call site
// keeps the one it was written with.
#pragma once

#include "common.hpp"

namespace itermvs {

// xor butterfly: every lane gets the sum
template <class T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// __shfl_down ladder: lane 0 holds the sum, the other lanes partial sums of no use
template <class T>
__device__ __forceinline__ T wave_sum_lane0(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// v of this lane and of the lanes below it
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// lanes of this wave below the caller with `on` set, and the wave's total
__device__ __forceinline__ uint32_t wave_rank(bool on, uint32_t& total) {
    const unsigned long long b = __ballot(on);
    total = (uint32_t)__popcll(b);
    const int lane = threadIdx.x & 63;
    return (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

// The items of the workgroup's threads before this one: `own` items of this thread, `inclusive_in_wave` = own + the items of the
// lanes below it (wave_inclusive_scan, or wave_rank + own).  Wave totals (lane 63's inclusive) go through LDS, one barrier.
// A kernel that calls it a second time puts a __syncthreads() between the calls: a wave that leaves the first call early would
// otherwise overwrite its total while a slower wave still reads it.
template <int kWaves, class T>
__device__ __forceinline__ T block_exclusive(T inclusive_in_wave, T own) {
    __shared__ T part[kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 63) part[wv] = inclusive_in_wave;
    __syncthreads();
    T before = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) before += k < wv ? part[k] : (T)0;
    return before + (inclusive_in_wave - own);
}

// ONE workgroup of kBlock threads turns c[0..n) into its exclusive prefix sums in place, kBlock at a time with a carry, and
// returns the total to every thread.  It ends with a barrier, so it may be called again at once (tsdf_scan_kernel: once per row).
// also(i) runs once for every i < n in the thread that owns item i, beside the load of c[i]: what a kernel sums over the same
// index on the side (fuse_points_scan_kernel; profiles/wave_ops/README.md has that kernel's time with a loop of its own instead).
template <class T, int kBlock, class Also>
__device__ __forceinline__ T block_scan_exclusive_chunked(T* __restrict__ c, uint32_t n, Also also) {
    __shared__ T wave_total[kBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T carry = 0;                                           // uniform: the chunks before this one
    for (uint32_t base = 0; base < n; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const T v = i < n ? c[i] : (T)0;
        if (i < n) also(i);
        const T inc = wave_inclusive_scan(v);
        if (lane == 63) wave_total[wv] = inc;
        __syncthreads();
        T before = 0, chunk = 0;
        for (int k = 0; k < kBlock / 64; ++k) {
            const T s = wave_total[k];
            before += k < wv ? s : (T)0;
            chunk += s;
        }
        if (i < n) c[i] = carry + before + (inc - v);
        carry += chunk;
        __syncthreads();                                   // wave_total is rewritten by the next chunk
    }
    return carry;
}

}  // namespace itermvs
