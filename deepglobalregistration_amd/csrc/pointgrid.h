// The uniform cell grid over the finite points of a target cloud that the radius search (gtmatch.hip) and the pair scoring
// (pairscore.hip) query: what a record holds and how a query walks it, shared as inline device functions; the kernels and
// the host function that build a call's grids are in pointgrid.hip.  ICP (o3d.hip) takes the bounding-box helpers only.
#pragma once
#include "dgr_internal.h"

__device__ __forceinline__ uint32_t dgr_ord_f32(float f) {   // f32 -> uint32 of the same order
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float dgr_unord_f32(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ bool dgr_finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// minima / maxima of three ordered-uint coordinates over the wave (every lane ends with the wave's)
__device__ __forceinline__ void dgr_bbox_wave_reduce(uint32_t lo[3], uint32_t hi[3]) {
  for (int s = 32; s >= 1; s >>= 1)
    for (int d = 0; d < 3; ++d) {
      lo[d] = min(lo[d], (uint32_t)__shfl_xor((int)lo[d], s, 64));
      hi[d] = max(hi[d], (uint32_t)__shfl_xor((int)hi[d], s, 64));
    }
}

struct DgrPointGrid {
  double gmin[3], cell;
  int64_t off;                 // first row of the cloud in the point array (set by the caller, like n)
  int64_t cell_base;           // first cell of the grid in the call's concatenated cell arrays
  int32_t n;                   // rows of the cloud
  int32_t gdim[3], ncell;      // ncell = 0: no finite point
  uint32_t bmin[3], bmax[3];   // ordered-uint bounding box of the finite points
};

// what dgr_point_grids_build hands back (arena memory of the call)
struct DgrPointGridSet {
  DgrPointGrid *grids;   // [ngrids], laid out
  int32_t *cell_start;   // [ncell + 1], cell_base of a grid + its cell -> first record in `sorted`
  float4 *sorted;        // per finite point (x, y, z, bits of the cloud-local row index), cell by cell
  int64_t ncell;         // cells of all grids
};

// Uploads host_grids (off and n set, the rest is filled in here), builds them over the rows of xyz and waits for the
// stream once (the cell total sizes the arrays).  `pin`: at least 8 bytes of the context's pinned buffer, asked for by the
// caller, who may need more of it later (a growth drops the contents).  `who` / `scope`: for the error message.
int dgr_point_grids_build(dgr_ctx *ctx, const float *xyz, DgrPointGrid *host_grids, int ngrids, double radius,
                          unsigned char *pin, const char *who, const char *scope, DgrPointGridSet *out, hipStream_t stream);

__device__ __forceinline__ int dgr_grid_cell_of(const DgrPointGrid &G, const float *q) {
  const int cx = (int)floor(((double)q[0] - G.gmin[0]) / G.cell), cy = (int)floor(((double)q[1] - G.gmin[1]) / G.cell),
            cz = (int)floor(((double)q[2] - G.gmin[2]) / G.cell);
  return (cz * G.gdim[1] + cy) * G.gdim[0] + cx;
}

// p = [R | t] s in float64 on the f32 row widened exactly.  The operation order is fixed and there is no fma (the pragma
// is lexical: it has to stand HERE), so that a host restatement gets the same bits.
__device__ __forceinline__ void dgr_pose_apply(const double *T, const float *s, double *px, double *py, double *pz) {
#pragma clang fp contract(off)
  const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
  *px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  *py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  *pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// f(q, d2) for every record q of the 27 cells around the finite point p, walked as 9 runs of up to 3 contiguous cells
// (the cells of a row of the grid are contiguous); d2 = |p - q|^2 in the same fixed order without fma.  Every point
// closer than the radius the grid was built for is among them.  The order inside a cell is whatever the build's atomic
// cursors gave: f must not depend on it.
template <class F>
__device__ __forceinline__ void dgr_grid_visit(const DgrPointGrid &G, const int32_t *starts, const float4 *sorted, double px,
                                               double py, double pz, F f) {
#pragma clang fp contract(off)
  // the query's cell, clamped to two cells outside the grid (farther queries cannot have a hit)
  const int cx = (int)fmin(fmax(floor((px - G.gmin[0]) / G.cell), -2.0), (double)G.gdim[0] + 1.0);
  const int cy = (int)fmin(fmax(floor((py - G.gmin[1]) / G.cell), -2.0), (double)G.gdim[1] + 1.0);
  const int cz = (int)fmin(fmax(floor((pz - G.gmin[2]) / G.cell), -2.0), (double)G.gdim[2] + 1.0);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, G.gdim[0] - 1);
  if (x0 > x1) return;
  const int32_t *st = starts + G.cell_base;
  for (int a = 0; a < 9; ++a) {
    const int zz = cz + a / 3 - 1, yy = cy + a % 3 - 1;
    if (zz < 0 || zz >= G.gdim[2] || yy < 0 || yy >= G.gdim[1]) continue;
    const int rowc = (zz * G.gdim[1] + yy) * G.gdim[0];
    const int32_t e1 = st[rowc + x1 + 1];
    for (int32_t e = st[rowc + x0]; e < e1; ++e) {
      const float4 q = sorted[e];
      const double ex = px - (double)q.x, ey = py - (double)q.y, ez = pz - (double)q.z;
      f(q, (ex * ex + ey * ey) + ez * ez);
    }
  }
}
