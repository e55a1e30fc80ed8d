// Builds the uniform point grids of pointgrid.h: bounding boxes, layout, and a counting sort of the finite points by cell.
#include "pointgrid.h"

#include <algorithm>

constexpr int PG_THREADS = 256;
constexpr int32_t PG_CELL_CAP = 1 << 20;   // cells per grid (the cell edge doubles until the grid fits)
constexpr int PG_MAX_Y = 65535;            // grids are the y dimension of the launches

__global__ void __launch_bounds__(PG_THREADS) pg_bbox_kernel(const float *__restrict__ xyz, DgrPointGrid *grids) {
  DgrPointGrid *G = grids + blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * PG_THREADS + threadIdx.x;
  if ((int64_t)blockIdx.x * PG_THREADS >= G->n) return;   // block-uniform
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (j < G->n) {
    const float *q = xyz + (G->off + j) * 3;
    if (dgr_finite3(q))
      for (int d = 0; d < 3; ++d) lo[d] = hi[d] = dgr_ord_f32(q[d]);
  }
  dgr_bbox_wave_reduce(lo, hi);
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; ++d) { atomicMin(&G->bmin[d], lo[d]); atomicMax(&G->bmax[d], hi[d]); }
}

// Cell edge >= radius (doubled until the grid fits PG_CELL_CAP), so that every point closer than the radius lies in the
// 27 cells around the query's.  The edge starts a hair ABOVE the radius: a query and a hit are then less than (1 - 1e-7)
// cells apart along every axis and the rounding of the two cell computations (~1e-10 cells at 2^20 cells per axis) cannot
// put them two cells apart.  Then the grids' cell ranges back to back (serial: the grids of a call are few).
__global__ void pg_layout_kernel(DgrPointGrid *grids, int ngrids, double radius, int64_t *total_cells) {
  for (int g = threadIdx.x; g < ngrids; g += blockDim.x) {
    DgrPointGrid *G = grids + g;
    G->ncell = 0;
    G->gdim[0] = G->gdim[1] = G->gdim[2] = 0;
    G->cell = radius;
    G->gmin[0] = G->gmin[1] = G->gmin[2] = 0.0;
    if (G->bmin[0] > G->bmax[0]) continue;   // no finite point
    double lo[3], hi[3];
    for (int d = 0; d < 3; ++d) { lo[d] = (double)dgr_unord_f32(G->bmin[d]); hi[d] = (double)dgr_unord_f32(G->bmax[d]); }
    double cell = radius * (1.0 + 1e-7);
    for (int tries = 0; tries < 2200; ++tries) {   // (2^2200 passes the exponent range: the loop ends by fitting)
      double total = 1.0;
      for (int d = 0; d < 3; ++d) total *= floor((hi[d] - lo[d]) / cell) + 1.0;
      if (total <= (double)PG_CELL_CAP) break;
      cell *= 2.0;
    }
    int64_t total = 1;
    for (int d = 0; d < 3; ++d) {
      G->gmin[d] = lo[d];
      G->gdim[d] = (int32_t)(floor((hi[d] - lo[d]) / cell) + 1.0);
      total *= G->gdim[d];
    }
    G->cell = cell;
    G->ncell = (int32_t)total;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t base = 0;
    for (int g = 0; g < ngrids; ++g) { grids[g].cell_base = base; base += grids[g].ncell; }
    *total_cells = base;
  }
}

// pass 1 (FILL = false): points per cell; pass 2: every finite point into its cell's range as (x, y, z, bits of the
// cloud-local row index), one 16-byte value.  The order inside a cell is whatever the atomic cursors give.
template <bool FILL>
__global__ void __launch_bounds__(PG_THREADS)
    pg_grid_kernel(const float *__restrict__ xyz, const DgrPointGrid *__restrict__ grids, int32_t *__restrict__ counts,
                   const int32_t *__restrict__ starts, float4 *__restrict__ sorted) {
  const DgrPointGrid &G = grids[blockIdx.y];
  const int64_t j = (int64_t)blockIdx.x * PG_THREADS + threadIdx.x;
  if (j >= G.n || G.ncell == 0) return;
  const float *q = xyz + (G.off + j) * 3;
  if (!dgr_finite3(q)) return;
  const int64_t c = G.cell_base + dgr_grid_cell_of(G, q);
  const int32_t k = atomicAdd(&counts[c], 1);
  if (FILL) sorted[starts[c] + k] = make_float4(q[0], q[1], q[2], __int_as_float((int32_t)j));
}

int dgr_point_grids_build(dgr_ctx *ctx, const float *xyz, DgrPointGrid *host_grids, int ngrids, double radius,
                          unsigned char *pin, const char *who, const char *scope, DgrPointGridSet *out, hipStream_t stream) {
  DgrArena &A = ctx->arena;
  int64_t max_n = 0, n_all = 0;
  for (int g = 0; g < ngrids; ++g) {
    DgrPointGrid &G = host_grids[g];
    for (int d = 0; d < 3; ++d) { G.bmin[d] = 0xffffffffu; G.bmax[d] = 0u; }
    max_n = std::max<int64_t>(max_n, G.n);
    n_all += G.n;
  }
  int64_t *total_cells;
  DGR_ALLOC(out->grids, A, DgrPointGrid, ngrids);
  DGR_ALLOC(total_cells, A, int64_t, 1);
  // `host_grids` is read by an asynchronous copy: the wait below comes before this function returns
  DGR_HIP_CHECK(hipMemcpyAsync(out->grids, host_grids, (size_t)ngrids * sizeof(DgrPointGrid), hipMemcpyHostToDevice, stream));
  const unsigned bx = (unsigned)dgr_ceil_div(max_n, PG_THREADS);   // (0: no grid has a row, and then no cell)
  for (int g0 = 0; g0 < ngrids && bx > 0; g0 += PG_MAX_Y)
    pg_bbox_kernel<<<dim3(bx, std::min(ngrids - g0, PG_MAX_Y)), PG_THREADS, 0, stream>>>(xyz, out->grids + g0);
  pg_layout_kernel<<<1, PG_THREADS, 0, stream>>>(out->grids, ngrids, radius, total_cells);
  DGR_LAUNCH_CHECK();
  // the cell count of the call sizes the grids' arrays (a 3DMatch fragment at 10-cm cells has ~10^5 cells, not the cap)
  DGR_HIP_CHECK(hipMemcpyAsync(pin, total_cells, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));
  const int64_t ncell = *reinterpret_cast<volatile int64_t *>(pin);
  DGR_REQUIRE(ncell >= 0 && ncell < INT32_MAX - 1, "%s: %lld grid cells in the %s", who, (long long)ncell, scope);

  int32_t *cell_count;
  DGR_ALLOC(cell_count, A, int32_t, ncell + 1);
  DGR_ALLOC(out->cell_start, A, int32_t, ncell + 1);
  DGR_ALLOC(out->sorted, A, float4, n_all);
  out->ncell = ncell;
  const size_t cell_bytes = (size_t)(ncell + 1) * sizeof(int32_t);
  DGR_HIP_CHECK(hipMemsetAsync(cell_count, 0, cell_bytes, stream));
  for (int g0 = 0; g0 < ngrids && ncell > 0; g0 += PG_MAX_Y)
    pg_grid_kernel<false><<<dim3(bx, std::min(ngrids - g0, PG_MAX_Y)), PG_THREADS, 0, stream>>>(xyz, out->grids + g0, cell_count,
                                                                                               nullptr, nullptr);
  DGR_CHECK(dgr_exclusive_scan_i32(A, cell_count, out->cell_start, ncell + 1, nullptr, stream));
  DGR_HIP_CHECK(hipMemsetAsync(cell_count, 0, cell_bytes, stream));   // the counts have been scanned: now the fill cursors
  for (int g0 = 0; g0 < ngrids && ncell > 0; g0 += PG_MAX_Y)
    pg_grid_kernel<true><<<dim3(bx, std::min(ngrids - g0, PG_MAX_Y)), PG_THREADS, 0, stream>>>(xyz, out->grids + g0, cell_count,
                                                                                              out->cell_start, out->sorted);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}
