// The one workgroup-wide exclusive scan of the library: coordmap.hip's scan kernels, gtmatch.hip's int64 offsets and the
// per-block output positions of tsdf.hip and tsdfmesh.hip all call it.
//
// dgr_block_exclusive<T, THREADS>(v, lds, &total) returns the sum of `v` over the threads below the caller and leaves the
// sum over all THREADS threads in *total (the same value in every thread).  Integer sums: exact in any grouping.
//
// Barrier contract:
//   * EVERY thread of the workgroup calls it, the same number of times -- it holds two __syncthreads(); a thread with
//     nothing to add passes 0.  blockDim.x == THREADS, a multiple of the wave size 64.
//   * `lds` is THREADS / 64 values of T in shared memory, the same pointer in every thread.  Nothing else may touch it
//     between a call's start and its return.
//   * The second barrier stands behind the last read of `lds`, so the function may be called again at once (a carry loop)
//     and the caller may return right after it.
#pragma once
#include <hip/hip_runtime.h>

template <typename T, int THREADS>
__device__ __forceinline__ T dgr_block_exclusive(T v, T *lds, T *total) {
  static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves of one workgroup");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T x = v;   // inclusive scan over the wave with shuffles, then the wave totals through LDS
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const T s = lds[w];
    if (w < wave) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}
