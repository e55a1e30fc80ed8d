// What tsdf.hip (fusion, crossings as points) and tsdfmesh.hip (the same crossings as mesh vertices) both state about a
// fused volume: one text, so that "same points, same order, same bits" holds by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// workgroups per block of the per-block kernels: a 16^3 block is four slabs of four z-layers (4 voxels per thread instead
// of 16: a fragment has a few hundred such blocks, too few workgroups of 16 serial voxels per thread to fill 256 CUs
// evenly).  Slabs are consecutive ranges of the voxel number l, so numbering the workgroups block-major keeps the order.
template <int B> struct TsdfSplit { static constexpr int value = B == 16 ? 4 : 1; };

// a voxel can end an edge with a crossing: observed often enough and not saturated
__device__ __forceinline__ bool tsdf_usable(float f, int32_t w, int min_weight) {
  return w >= min_weight && f >= -0.98f && f < 0.98f;
}

// p = the zero crossing on the +a edge of voxel lc of block bc, whose ends hold f0 (the voxel) and f1 (its +a neighbour);
// returns the crossing's fraction of the edge.  The arithmetic is DEFINED without fma (include/dgr_hip.h).
template <int B>
__device__ __forceinline__ double tsdf_crossing_point(const int32_t bc[3], const int lc[3], int a, float f0, float f1,
                                                      double voxel, double p[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 3; ++e) p[e] = ((double)(bc[e] * B + lc[e]) + 0.5) * voxel;
  const double r0 = fabs((double)f0), r1 = fabs((double)f1);
  const double r = r0 / (r0 + r1);
  p[a] = p[a] + voxel * r;
  return r;
}

// c = the colour of that crossing in [0, 1]: the two ends' mean colours (rgb_sum / weight, exact integer sums over the
// frames that updated the voxel) blended with the very r that places the point.  s0 / s1 point at the three sums of the
// voxel and of its +a neighbour; w0, w1 >= min_weight >= 1.  DEFINED without fma, like the position.
__device__ __forceinline__ void tsdf_crossing_color(const int32_t *__restrict__ s0, int32_t w0, const int32_t *__restrict__ s1,
                                                    int32_t w1, double r, double c[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double m0 = (double)s0[e] / (double)w0, m1 = (double)s1[e] / (double)w1;
    c[e] = (m0 + r * (m1 - m0)) / 255.0;
  }
}
