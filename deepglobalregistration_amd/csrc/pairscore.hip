// Geometric fit of registered pairs of a fragment bank: for every directed pair (source fragment, target fragment) and
// its pose, the sums over the source rows that have a partner within the radius --
//   n, sum d^2, sum q (3), sum q q^T (upper triangle, 6)        q = the partner, a target point
// from which the host derives what the reference and Open3D report per pair: the overlap ratio
// (util/pointcloud.py:72-80, compute_overlap_ratio: n / rows in both directions), fitness / inlier_rmse
// (RegistrationResult) and the 6x6 information matrix (GetInformationMatrixFromPointClouds, the .info record of the
// 3DMatch / Redwood benchmark).  Open3D is absent here: those formulas are restated.
//
// The partner of a source row is the target row minimising (d^2, j) among those with d^2 < radius^2, STRICTLY: the first
// entry dgr_radius_pairs_batch(K = 1) lists for the row, by the same pose, the same walk and the same float64 distances as
// that call (dgr_pose_apply, dgr_grid_visit; csrc/pointgrid.h).  Unlike that call, this one writes no pair list and builds
// ONE uniform grid per fragment that occurs as a target, whatever the number of pairs it is the target of.
//
// Determinism: a source row's eleven terms are a function of the input alone (the order of a grid cell's entries, which
// the atomic cursors decide, does not enter a minimum over (d^2, j)); they are summed per wave by a shuffle butterfly, per
// block over the four waves in order, per pair over its blocks in a fixed strided order -- no floating-point atomics.  The
// tree depends on the source fragment's row count alone, so two runs agree bit for bit and a pair's values do not depend
// on the other pairs of the call.
#include "pointgrid.h"

#include <algorithm>
#include <cmath>
#include <cstring>

constexpr int PS_THREADS = 256;
constexpr int PS_WIDTH = DGR_SCORE_WIDTH;
constexpr int PS_MAX_Y = 65535;   // pairs are the y dimension of the launches

struct PsPair {
  double T[12];                // [R | t] row-major 3x4
  int64_t off0;                // first row of the source fragment in the bank
  int64_t part_base;           // first of the pair's per-block partial records
  int32_t n0;                  // rows of the source fragment
  int32_t grid;                // index of the target fragment's grid
};

// One thread per source row, the pair is blockIdx.y: pose and grid are block-uniform.  The row's partner is the minimum
// over (d^2, j) of the hits in the 27 cells around the transformed row; its eleven terms are reduced over the block and
// written as the pair's partial record number blockIdx.x.
__global__ void __launch_bounds__(PS_THREADS)
    ps_query_kernel(const float *__restrict__ xyz, const PsPair *__restrict__ pairs, const DgrPointGrid *__restrict__ grids,
                    const int32_t *__restrict__ starts, const float4 *__restrict__ sorted, double r2,
                    double *__restrict__ partial) {
#pragma clang fp contract(off)   // the sums are DEFINED without fma, like the pose and the distances (pointgrid.h)
  __shared__ double red[PS_THREADS / 64][PS_WIDTH];
  const PsPair *P = pairs + blockIdx.y;
  if ((int64_t)blockIdx.x * PS_THREADS >= P->n0) return;   // block-uniform
  const DgrPointGrid &G = grids[P->grid];
  const int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  double best = r2;
  int32_t bj = -1;
  float bx = 0.f, by = 0.f, bz = 0.f;
  if (i < P->n0 && G.ncell > 0) {
    double px, py, pz;
    dgr_pose_apply(P->T, xyz + (P->off0 + i) * 3, &px, &py, &pz);
    if (isfinite(px) && isfinite(py) && isfinite(pz))   // (a non-finite source row transforms to non-finite)
      dgr_grid_visit(G, starts, sorted, px, py, pz, [&](const float4 &q, double d2) {
        const int32_t j = __float_as_int(q.w);
        // best starts at r^2 with no partner: the first hit must be STRICTLY below it; then (d^2, j) ascending
        if (d2 < best || (d2 == best && bj >= 0 && j < bj)) { best = d2; bj = j; bx = q.x; by = q.y; bz = q.z; }
      });
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
  std::vector<DgrPointGrid> hgrids;
  for (int f = 0; f < nfrag; ++f) {
    if (grid_of[f] < 0) continue;
    grid_of[f] = (int32_t)hgrids.size();
    DgrPointGrid G;
    memset(&G, 0, sizeof(G));
    G.off = bank_off[f];
    G.n = (int32_t)(bank_off[f + 1] - bank_off[f]);
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
  PsPair *pairs;
  double *partial, *sums;
  DGR_ALLOC(pairs, A, PsPair, npairs);
  DGR_ALLOC(partial, A, double, nparts * PS_WIDTH);
  DGR_ALLOC(sums, A, double, (size_t)npairs * PS_WIDTH);
  // `hpairs` is read by an asynchronous copy: it lives until this function returns, and it does not return before the
  // stream is idle
  DGR_HIP_CHECK(hipMemcpyAsync(pairs, hpairs.data(), (size_t)npairs * sizeof(PsPair), hipMemcpyHostToDevice, stream));
  DgrPointGridSet grid;
  DGR_CHECK(dgr_point_grids_build(ctx, bank_xyz, hgrids.data(), ngrids, radius, pin, "dgr_score_pairs", "call", &grid, stream));
  const double r2 = radius * radius;
  for (int p0 = 0; p0 < npairs; p0 += PS_MAX_Y) {   // (a launch takes 65535 pairs)
    const int np = std::min(npairs - p0, PS_MAX_Y);
    int64_t max0 = 0;
    for (int p = p0; p < p0 + np; ++p) max0 = std::max<int64_t>(max0, hpairs[p].n0);
    ps_query_kernel<<<dim3((unsigned)dgr_ceil_div(max0, PS_THREADS), np), PS_THREADS, 0, stream>>>(bank_xyz, pairs + p0, grid.grids,
                                                                                                  grid.cell_start, grid.sorted, r2, partial);
  }
  ps_final_kernel<<<npairs, 64, 0, stream>>>(pairs, partial, sums);
  DGR_LAUNCH_CHECK();
  DGR_HIP_CHECK(hipMemcpyAsync(pin + 64, sums, out_bytes, hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // like every entry point that returns host values, this one synchronises
  memcpy(sums_out, pin + 64, out_bytes);
  return DGR_OK;
}
