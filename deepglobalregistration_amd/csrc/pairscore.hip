// Geometric fit of registered pairs of a fragment bank: for every directed pair (source fragment, target fragment) and
// its pose, the sums over the source rows that have a partner within the radius --
//   n, sum d^2, sum q (3), sum q q^T (upper triangle, 6)        q = the partner, a target point
// from which the host derives what the reference and Open3D report per pair: the overlap ratio
// (util/pointcloud.py:72-80, compute_overlap_ratio: n / rows in both directions), fitness / inlier_rmse
// (RegistrationResult) and the 6x6 information matrix (GetInformationMatrixFromPointClouds, the .info record of the
// 3DMatch / Redwood benchmark).  Open3D is absent here: those formulas are restated.
//
// The partner of a source row is the target row minimising (d^2, j) among those with d^2 < radius^2, STRICTLY: the first
// entry dgr_radius_pairs_batch(K = 1) lists for the row, in the same float64 arithmetic on the f32 points widened exactly
// (fixed operation order, no fma; csrc/gtmatch.hip).  Unlike that call, this one writes no pair list and builds ONE uniform
// grid per fragment that occurs as a target, whatever the number of pairs it is the target of.
//
// Determinism: a source row's eleven terms are a function of the input alone (the order of a grid cell's entries, which
// the atomic cursors decide, does not enter a minimum over (d^2, j)); they are summed per wave by a shuffle butterfly, per
// block over the four waves in order, per pair over its blocks in a fixed strided order -- no floating-point atomics.  The
// tree depends on the source fragment's row count alone, so two runs agree bit for bit and a pair's values do not depend
// on the other pairs of the call.
#include "dgr_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

constexpr int PS_THREADS = 256;
constexpr int PS_WIDTH = DGR_SCORE_WIDTH;
constexpr int32_t PS_CELL_CAP = 1 << 20;   // grid cells per target fragment (the cell edge doubles until the grid fits)
constexpr int PS_MAX_Y = 65535;            // pairs (grids) are the y dimension of the launches

// the uniform grid over the finite points of one target fragment
struct PsGrid {
  double gmin[3], cell;
  int64_t off;                 // first row of the fragment in the bank
  int64_t cell_base;           // first cell of the grid in the call's concatenated cell arrays
  int32_t n;                   // rows of the fragment
  int32_t gdim[3], ncell;      // ncell = 0: no finite point
  uint32_t bmin[3], bmax[3];   // ordered-uint bounding box of the finite points
};

struct PsPair {
  double T[12];                // [R | t] row-major 3x4
  int64_t off0;                // first row of the source fragment in the bank
  int64_t part_base;           // first of the pair's per-block partial records
  int32_t n0;                  // rows of the source fragment
  int32_t grid;                // index of the target fragment's grid
};

__device__ __forceinline__ uint32_t ps_ord_f32(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ps_unord_f32(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ bool ps_finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__global__ void __launch_bounds__(PS_THREADS) ps_bbox_kernel(const float *__restrict__ xyz, PsGrid *grids) {
  PsGrid *G = grids + blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if ((int64_t)blockIdx.x * PS_THREADS >= G->n) return;   // block-uniform
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (j < G->n) {
    const float *q = xyz + (G->off + j) * 3;
    if (ps_finite3(q))
      for (int d = 0; d < 3; ++d) lo[d] = hi[d] = ps_ord_f32(q[d]);
  }
  for (int s = 32; s >= 1; s >>= 1)
    for (int d = 0; d < 3; ++d) {
      lo[d] = min(lo[d], (uint32_t)__shfl_xor((int)lo[d], s, 64));
      hi[d] = max(hi[d], (uint32_t)__shfl_xor((int)hi[d], s, 64));
    }
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; ++d) { atomicMin(&G->bmin[d], lo[d]); atomicMax(&G->bmax[d], hi[d]); }
}

// Cell edge >= radius (doubled until the fragment's grid fits PS_CELL_CAP), so that every target point closer than the
// radius lies in the 27 cells around the query's.  The edge starts a hair ABOVE the radius: a query and a hit are then less
// than (1 - 1e-7) cells apart along every axis and the rounding of the two cell computations (~1e-10 cells at 2^20 cells
// per axis) cannot put them two cells apart.  Then the grids' cell ranges back to back (serial: one entry per fragment).
__global__ void ps_layout_kernel(PsGrid *grids, int ngrids, double radius, int64_t *total_cells) {
  for (int g = threadIdx.x; g < ngrids; g += blockDim.x) {
    PsGrid *G = grids + g;
    G->ncell = 0;
    G->gdim[0] = G->gdim[1] = G->gdim[2] = 0;
    G->cell = radius;
    G->gmin[0] = G->gmin[1] = G->gmin[2] = 0.0;
    if (G->bmin[0] > G->bmax[0]) continue;   // no finite point
    double lo[3], hi[3];
    for (int d = 0; d < 3; ++d) { lo[d] = (double)ps_unord_f32(G->bmin[d]); hi[d] = (double)ps_unord_f32(G->bmax[d]); }
    double cell = radius * (1.0 + 1e-7);
    for (int tries = 0; tries < 2200; ++tries) {   // (2^2200 passes the exponent range: the loop ends by fitting)
      double total = 1.0;
      for (int d = 0; d < 3; ++d) total *= floor((hi[d] - lo[d]) / cell) + 1.0;
      if (total <= (double)PS_CELL_CAP) break;
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

// grid build, pass 1 (FILL = false): points per cell; pass 2: every finite point into its cell's range as
// (x, y, z, bits of the fragment-local row index), one 16-byte value.  The order inside a cell is whatever the atomic
// cursors give: the (d^2, j) minimum of the search does not depend on it.
template <bool FILL>
__global__ void __launch_bounds__(PS_THREADS)
    ps_grid_kernel(const float *__restrict__ xyz, const PsGrid *__restrict__ grids, int32_t *__restrict__ counts,
                   const int32_t *__restrict__ starts, float4 *__restrict__ sorted) {
  const PsGrid *G = grids + blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (j >= G->n || G->ncell == 0) return;
  const float *q = xyz + (G->off + j) * 3;
  if (!ps_finite3(q)) return;
  const int cx = (int)floor(((double)q[0] - G->gmin[0]) / G->cell), cy = (int)floor(((double)q[1] - G->gmin[1]) / G->cell),
            cz = (int)floor(((double)q[2] - G->gmin[2]) / G->cell);
  const int64_t c = G->cell_base + ((int64_t)(cz * G->gdim[1] + cy) * G->gdim[0] + cx);
  const int32_t k = atomicAdd(&counts[c], 1);
  if (FILL) sorted[starts[c] + k] = make_float4(q[0], q[1], q[2], __int_as_float((int32_t)j));
}

// One thread per source row, the pair is blockIdx.y: pose and grid are block-uniform.  The row's partner is the minimum
// over (d^2, j) of the hits in the 27 cells around the transformed row, walked as 9 runs of up to 3 contiguous cells; its
// eleven terms are reduced over the block and written as the pair's partial record number blockIdx.x.
__global__ void __launch_bounds__(PS_THREADS)
    ps_query_kernel(const float *__restrict__ xyz, const PsPair *__restrict__ pairs, const PsGrid *__restrict__ grids,
                    const int32_t *__restrict__ starts, const float4 *__restrict__ sorted, double r2,
                    double *__restrict__ partial) {
#pragma clang fp contract(off)   // the pose and the distances are DEFINED without fma (see the head of this file)
  __shared__ double red[PS_THREADS / 64][PS_WIDTH];
  const PsPair *P = pairs + blockIdx.y;
  if ((int64_t)blockIdx.x * PS_THREADS >= P->n0) return;   // block-uniform
  const PsGrid *G = grids + P->grid;
  const int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  double best = r2;
  int32_t bj = -1;
  float bx = 0.f, by = 0.f, bz = 0.f;
  if (i < P->n0 && G->ncell > 0) {
    const float *s = xyz + (P->off0 + i) * 3;
    const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
    const double px = ((P->T[0] * x + P->T[1] * y) + P->T[2] * z) + P->T[3];
    const double py = ((P->T[4] * x + P->T[5] * y) + P->T[6] * z) + P->T[7];
    const double pz = ((P->T[8] * x + P->T[9] * y) + P->T[10] * z) + P->T[11];
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {   // (a non-finite source row transforms to non-finite)
      // the query's cell, clamped to two cells outside the grid (farther queries cannot have a hit)
      const int cx = (int)fmin(fmax(floor((px - G->gmin[0]) / G->cell), -2.0), (double)G->gdim[0] + 1.0);
      const int cy = (int)fmin(fmax(floor((py - G->gmin[1]) / G->cell), -2.0), (double)G->gdim[1] + 1.0);
      const int cz = (int)fmin(fmax(floor((pz - G->gmin[2]) / G->cell), -2.0), (double)G->gdim[2] + 1.0);
      const int x0 = max(cx - 1, 0), x1 = min(cx + 1, G->gdim[0] - 1);   // the cells of a row of the grid are contiguous
      const int32_t *st = starts + G->cell_base;
      if (x0 <= x1)
        for (int a = 0; a < 9; ++a) {
          const int zz = cz + a / 3 - 1, yy = cy + a % 3 - 1;
          if (zz < 0 || zz >= G->gdim[2] || yy < 0 || yy >= G->gdim[1]) continue;
          const int rowc = (zz * G->gdim[1] + yy) * G->gdim[0];
          const int32_t e1 = st[rowc + x1 + 1];
          for (int32_t e = st[rowc + x0]; e < e1; ++e) {
            const float4 q = sorted[e];
            const double ex = px - (double)q.x, ey = py - (double)q.y, ez = pz - (double)q.z;
            const double d2 = (ex * ex + ey * ey) + ez * ez;
            const int32_t j = __float_as_int(q.w);
            // best starts at r^2 with no partner: the first hit must be STRICTLY below it; then (d^2, j) ascending
            if (d2 < best || (d2 == best && bj >= 0 && j < bj)) { best = d2; bj = j; bx = q.x; by = q.y; bz = q.z; }
          }
        }
    }
  }
  double v[PS_WIDTH];
  {
    const bool has = bj >= 0;
    const double qx = has ? (double)bx : 0.0, qy = has ? (double)by : 0.0, qz = has ? (double)bz : 0.0;
    v[0] = has ? 1.0 : 0.0;
    v[1] = has ? best : 0.0;
    v[2] = qx; v[3] = qy; v[4] = qz;
    v[5] = qx * qx; v[6] = qx * qy; v[7] = qx * qz;   // (products of widened f32: exact in f64)
    v[8] = qy * qy; v[9] = qy * qz; v[10] = qz * qz;
  }
#pragma unroll
  for (int k = 0; k < PS_WIDTH; ++k) {
    double t = v[k];
    for (int s = 32; s >= 1; s >>= 1) t += __shfl_xor(t, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < PS_WIDTH) {
    double t = red[0][threadIdx.x];
    for (int w = 1; w < PS_THREADS / 64; ++w) t += red[w][threadIdx.x];
    partial[(P->part_base + blockIdx.x) * PS_WIDTH + threadIdx.x] = t;
  }
}

// one wave per pair: lane l sums the partial records l, l + 64, ... of the pair in order, then the butterfly
__global__ void __launch_bounds__(64)
    ps_final_kernel(const PsPair *__restrict__ pairs, const double *__restrict__ partial, double *__restrict__ sums) {
#pragma clang fp contract(off)
  const PsPair *P = pairs + blockIdx.x;
  const int64_t nb = ((int64_t)P->n0 + PS_THREADS - 1) / PS_THREADS;
  const double *rec = partial + P->part_base * PS_WIDTH;
  for (int k = 0; k < PS_WIDTH; ++k) {
    double t = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += 64) t += rec[b * PS_WIDTH + k];
    for (int s = 32; s >= 1; s >>= 1) t += __shfl_xor(t, s, 64);
    if (threadIdx.x == 0) sums[(int64_t)blockIdx.x * PS_WIDTH + k] = t;
  }
}

extern "C" int dgr_score_pairs(dgr_ctx *ctx, const float *bank_xyz, const int64_t *bank_off, int nfrag,
                               const int32_t *pair_ids, int npairs, const double *T, double radius, double *sums_out,
                               dgr_stream stream_) {
  // argument errors first: nothing has touched the device when one of them is reported
  DGR_REQUIRE(ctx && bank_xyz && bank_off && pair_ids && T && sums_out, "dgr_score_pairs: NULL argument");
  DGR_REQUIRE(npairs >= 1, "dgr_score_pairs: npairs = %d", npairs);
  DGR_REQUIRE(nfrag >= 1, "dgr_score_pairs: nfrag = %d", nfrag);
  DGR_REQUIRE(radius > 0.0 && std::isfinite(radius), "dgr_score_pairs: radius must be positive and finite");
  DGR_REQUIRE(std::isfinite(radius * radius), "dgr_score_pairs: radius^2 overflows");
  DGR_REQUIRE(bank_off[0] >= 0, "dgr_score_pairs: bank_off[0] = %lld", (long long)bank_off[0]);
  for (int f = 0; f < nfrag; ++f)
    DGR_REQUIRE(bank_off[f + 1] > bank_off[f], "dgr_score_pairs: fragment %d of the bank is empty", f);
  DGR_REQUIRE(bank_off[nfrag] < INT32_MAX, "dgr_score_pairs: more than 2^31 rows");
  for (int p = 0; p < npairs; ++p) {
    for (int s = 0; s < 2; ++s)
      DGR_REQUIRE(pair_ids[2 * p + s] >= 0 && pair_ids[2 * p + s] < nfrag, "dgr_score_pairs: pair %d: fragment id %d outside [0, %d)",
                  p, pair_ids[2 * p + s], nfrag);
    for (int k = 0; k < 12; ++k)
      DGR_REQUIRE(std::isfinite(T[(size_t)p * 16 + k]), "dgr_score_pairs: pair %d: non-finite pose", p);
  }

  // one grid per fragment that occurs as a target, in fragment order; the pairs' records
  std::vector<int32_t> grid_of(nfrag, -1);
  for (int p = 0; p < npairs; ++p) grid_of[pair_ids[2 * p + 1]] = 0;
  std::vector<PsGrid> hgrids;
  int64_t max1 = 0, n1_all = 0;
  for (int f = 0; f < nfrag; ++f) {
    if (grid_of[f] < 0) continue;
    grid_of[f] = (int32_t)hgrids.size();
    PsGrid G;
    memset(&G, 0, sizeof(G));
    G.off = bank_off[f];
    G.n = (int32_t)(bank_off[f + 1] - bank_off[f]);
    for (int d = 0; d < 3; ++d) { G.bmin[d] = 0xffffffffu; G.bmax[d] = 0u; }
    max1 = std::max<int64_t>(max1, G.n);
    n1_all += G.n;
    hgrids.push_back(G);
  }
  const int ngrids = (int)hgrids.size();
  std::vector<PsPair> hpairs(npairs);
  int64_t nparts = 0;
  for (int p = 0; p < npairs; ++p) {
    PsPair &P = hpairs[p];
    memset(&P, 0, sizeof(P));
    memcpy(P.T, T + (size_t)p * 16, 12 * sizeof(double));
    const int32_t f0 = pair_ids[2 * p];
    P.off0 = bank_off[f0];
    P.n0 = (int32_t)(bank_off[f0 + 1] - bank_off[f0]);
    P.grid = grid_of[pair_ids[2 * p + 1]];
    P.part_base = nparts;
    nparts += dgr_ceil_div(P.n0, PS_THREADS);
  }

  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  const size_t out_bytes = (size_t)npairs * PS_WIDTH * sizeof(double);
  unsigned char *pin;   // [0, 64): the cell total; from 64: the sums (asked for at once: a growth drops the contents)
  DGR_CHECK(dgr_ctx_pinned(ctx, 64 + out_bytes, &pin));
  PsGrid *grids;
  PsPair *pairs;
  int64_t *total_cells;
  double *partial, *sums;
  DGR_ALLOC(grids, A, PsGrid, ngrids);
  DGR_ALLOC(pairs, A, PsPair, npairs);
  DGR_ALLOC(total_cells, A, int64_t, 1);
  DGR_ALLOC(partial, A, double, nparts * PS_WIDTH);
  DGR_ALLOC(sums, A, double, (size_t)npairs * PS_WIDTH);
  // `hgrids` and `hpairs` are read by asynchronous copies: they live until this function returns, and it does not return
  // before the stream is idle
  DGR_HIP_CHECK(hipMemcpyAsync(grids, hgrids.data(), (size_t)ngrids * sizeof(PsGrid), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(pairs, hpairs.data(), (size_t)npairs * sizeof(PsPair), hipMemcpyHostToDevice, stream));
  const unsigned bx1 = (unsigned)dgr_ceil_div(max1, PS_THREADS);
  for (int g0 = 0; g0 < ngrids; g0 += PS_MAX_Y)
    ps_bbox_kernel<<<dim3(bx1, std::min(ngrids - g0, PS_MAX_Y)), PS_THREADS, 0, stream>>>(bank_xyz, grids + g0);
  ps_layout_kernel<<<1, PS_THREADS, 0, stream>>>(grids, ngrids, radius, total_cells);
  DGR_LAUNCH_CHECK();
  // the cell count of the call sizes the grids' arrays (a 3DMatch fragment at 10-cm cells has ~10^5 cells, not the cap)
  DGR_HIP_CHECK(hipMemcpyAsync(pin, total_cells, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));
  const int64_t ncell = *reinterpret_cast<volatile int64_t *>(pin);
  DGR_REQUIRE(ncell >= 0 && ncell < INT32_MAX - 1, "dgr_score_pairs: %lld grid cells in the call", (long long)ncell);

  int32_t *cell_count, *cell_start;
  float4 *sorted;
  DGR_ALLOC(cell_count, A, int32_t, ncell + 1);
  DGR_ALLOC(cell_start, A, int32_t, ncell + 1);
  DGR_ALLOC(sorted, A, float4, n1_all);
  const size_t cell_bytes = (size_t)(ncell + 1) * sizeof(int32_t);
  DGR_HIP_CHECK(hipMemsetAsync(cell_count, 0, cell_bytes, stream));
  if (ncell > 0)
    for (int g0 = 0; g0 < ngrids; g0 += PS_MAX_Y)
      ps_grid_kernel<false><<<dim3(bx1, std::min(ngrids - g0, PS_MAX_Y)), PS_THREADS, 0, stream>>>(bank_xyz, grids + g0, cell_count,
                                                                                                 nullptr, nullptr);
  DGR_CHECK(dgr_exclusive_scan_i32(A, cell_count, cell_start, ncell + 1, nullptr, stream));
  DGR_HIP_CHECK(hipMemsetAsync(cell_count, 0, cell_bytes, stream));   // the counts have been scanned: now the fill cursors
  if (ncell > 0)
    for (int g0 = 0; g0 < ngrids; g0 += PS_MAX_Y)
      ps_grid_kernel<true><<<dim3(bx1, std::min(ngrids - g0, PS_MAX_Y)), PS_THREADS, 0, stream>>>(bank_xyz, grids + g0, cell_count,
                                                                                                cell_start, sorted);
  const double r2 = radius * radius;
  for (int p0 = 0; p0 < npairs; p0 += PS_MAX_Y) {   // (a launch takes 65535 pairs)
    const int np = std::min(npairs - p0, PS_MAX_Y);
    int64_t max0 = 0;
    for (int p = p0; p < p0 + np; ++p) max0 = std::max<int64_t>(max0, hpairs[p].n0);
    ps_query_kernel<<<dim3((unsigned)dgr_ceil_div(max0, PS_THREADS), np), PS_THREADS, 0, stream>>>(bank_xyz, pairs + p0, grids,
                                                                                                  cell_start, sorted, r2, partial);
  }
  ps_final_kernel<<<npairs, 64, 0, stream>>>(pairs, partial, sums);
  DGR_LAUNCH_CHECK();
  DGR_HIP_CHECK(hipMemcpyAsync(pin + 64, sums, out_bytes, hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // like every entry point that returns host values, this one synchronises
  memcpy(sums_out, pin + 64, out_bytes);
  return DGR_OK;
}
