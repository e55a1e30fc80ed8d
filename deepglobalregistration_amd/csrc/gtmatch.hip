// Ground-truth matches and inlier validation counts -- what the reference computes on the host to judge its networks:
//   * the ground-truth correspondence set of a pair   (util/pointcloud.py:83-96, get_matching_indices: a Python loop of
//     Open3D KD-tree radius queries; the `correspondences` entry of every collated batch, dataloader/base_loader.py)
//   * the correctness label of every putative match   (core/correspondence.py:14-53, _hash + np.isin)
//   * the confusion counts of the inlier weights      (core/trainer.py:430-437)
// Open3D is absent here.  The radius search restates what o3d.geometry.KDTreeFlann.search_radius_vector_3d (FLANN radius
// search, sorted) returns: every target point with squared distance STRICTLY below radius^2, ascending by distance; equal
// distances are ordered by the smaller index here (FLANN leaves them in tree order), which makes the list a function of
// the input alone.  The transformation and the distances are float64 on the f32 points widened exactly, in a fixed
// operation order without fma, so that a host restatement (tests, tests/golden/make_golden_gt_match.py) gets the same bits.
#include "hash.h"
#include "pointgrid.h"
#include "scan.h"

#include <cmath>
#include <cstring>

constexpr int GT_THREADS = 256;
constexpr int GT_MAX_PAIRS = 65535;   // pairs are the y dimension of the launches

// per pair: pose and source rows; the uniform grid over the pair's finite target points is grid number p of the call
struct GtPair {
  double T[12];                // [R | t] row-major 3x4
  int64_t off0;                // first row of the pair in xyz0
  int32_t n0;
};

// One thread per source row.  FILL = false: the number of hits (capped at K when K > 0).  FILL = true: every hit whose rank
// by (d^2, j) among the row's hits is below the cap goes to pairs_out[row_off[row] + rank] -- the rank comes from a second
// walk over the same cells, so a row needs no list of its hits (no per-thread array, no scratch); quadratic in the
// candidates of the 27 cells, a few dozen on voxelised clouds.  Neighbouring threads own neighbouring output segments.
template <bool FILL>
__global__ void __launch_bounds__(GT_THREADS)
    gt_radius_kernel(const float *__restrict__ xyz0, const GtPair *__restrict__ pairs, const DgrPointGrid *__restrict__ grids,
                     const int32_t *__restrict__ starts, const float4 *__restrict__ sorted, double r2, int32_t K,
                     int32_t *__restrict__ counts_out, const int64_t *__restrict__ row_off, longlong2 *__restrict__ pairs_out) {
  const GtPair *P = pairs + blockIdx.y;
  const DgrPointGrid &G = grids[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (i >= P->n0) return;
  const int64_t row = P->off0 + i;
  double px, py, pz;
  dgr_pose_apply(P->T, xyz0 + row * 3, &px, &py, &pz);
  int32_t n = 0;
  if (G.ncell > 0 && isfinite(px) && isfinite(py) && isfinite(pz)) {   // (a non-finite source row transforms to non-finite)
    const int64_t out0 = FILL ? row_off[row] : 0;
    dgr_grid_visit(G, starts, sorted, px, py, pz, [&](const float4 &q, double d2) {
      if (!(d2 < r2)) return;
      if (!FILL) { ++n; return; }
      const int32_t j = __float_as_int(q.w);
      int32_t rank = 0;
      dgr_grid_visit(G, starts, sorted, px, py, pz, [&](const float4 &o, double o2) {
        rank += (o2 < d2 || (o2 == d2 && __float_as_int(o.w) < j)) ? 1 : 0;   // (o2 <= d2 < r2: a hit itself)
      });
      if (K == 0 || rank < K) pairs_out[out0 + rank] = make_longlong2((long long)i, (long long)j);
    });
  }
  if (!FILL) counts_out[row] = (K > 0 && n > K) ? K : n;
}

// ---- exclusive scan of the int32 row counts into int64 offsets [n + 1] (the total can pass 2^31) ---------------------
constexpr int GT_SCAN_ROWS = 1024;   // rows per block: 256 threads x 4 consecutive rows

__global__ void __launch_bounds__(GT_THREADS) gt_scan_sums_kernel(const int32_t *__restrict__ counts, int64_t n, int64_t *bsum) {
  const int64_t r0 = (int64_t)blockIdx.x * GT_SCAN_ROWS + threadIdx.x * 4;
  int64_t v = 0;
  for (int k = 0; k < 4; ++k) v += (r0 + k < n) ? counts[r0 + k] : 0;
  __shared__ int64_t lds[GT_THREADS / 64];
  int64_t total;
  dgr_block_exclusive<int64_t, GT_THREADS>(v, lds, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ void __launch_bounds__(GT_THREADS) gt_scan_blocks_kernel(int64_t *bsum, int nblocks, int64_t *total_out) {
  __shared__ int64_t lds[GT_THREADS / 64];
  int64_t carry = 0;
  for (int b0 = 0; b0 < nblocks; b0 += GT_THREADS) {
    const int b = b0 + threadIdx.x;
    const int64_t v = b < nblocks ? bsum[b] : 0;
    int64_t total;
    const int64_t ex = dgr_block_exclusive<int64_t, GT_THREADS>(v, lds, &total);
    if (b < nblocks) bsum[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}
__global__ void __launch_bounds__(GT_THREADS)
    gt_scan_final_kernel(const int32_t *__restrict__ counts, int64_t n, const int64_t *__restrict__ bsum,
                         const int64_t *__restrict__ total, int64_t *__restrict__ row_off) {
  const int64_t r0 = (int64_t)blockIdx.x * GT_SCAN_ROWS + threadIdx.x * 4;
  int32_t c[4];
  int64_t v = 0;
  for (int k = 0; k < 4; ++k) { c[k] = (r0 + k < n) ? counts[r0 + k] : 0; v += c[k]; }
  __shared__ int64_t lds[GT_THREADS / 64];
  int64_t unused;
  int64_t at = bsum[blockIdx.x] + dgr_block_exclusive<int64_t, GT_THREADS>(v, lds, &unused);
  for (int k = 0; k < 4; ++k) {
    if (r0 + k < n) row_off[r0 + k] = at;
    at += c[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) row_off[n] = *total;
}

static bool gt_offsets_ok(const int64_t *off, int npairs) {
  if (off[0] != 0) return false;
  for (int p = 0; p < npairs; ++p)
    if (off[p + 1] < off[p]) return false;
  return true;
}

extern "C" int dgr_radius_pairs_batch(dgr_ctx *ctx, const float *xyz0, const int64_t *off0, const float *xyz1,
                                      const int64_t *off1, int npairs, const double *T, double radius, int K,
                                      int32_t *counts_out, int64_t *pairs_out, int64_t capacity, int64_t *total_out,
                                      dgr_stream stream_) {
  // argument errors first: nothing has touched the device when one of them is reported
  DGR_REQUIRE(ctx && off0 && off1 && T && total_out, "dgr_radius_pairs_batch: NULL argument");
  DGR_REQUIRE(npairs >= 1 && npairs <= GT_MAX_PAIRS, "dgr_radius_pairs_batch: npairs = %d (1..%d)", npairs, GT_MAX_PAIRS);
  DGR_REQUIRE(radius > 0.0 && std::isfinite(radius), "dgr_radius_pairs_batch: radius must be positive and finite");
  DGR_REQUIRE(std::isfinite(radius * radius), "dgr_radius_pairs_batch: radius^2 overflows");
  DGR_REQUIRE(K >= 0, "dgr_radius_pairs_batch: K = %d (0 = no cap)", K);
  DGR_REQUIRE(gt_offsets_ok(off0, npairs) && gt_offsets_ok(off1, npairs),
              "dgr_radius_pairs_batch: offsets must start at 0 and not decrease");
  const int64_t n0_all = off0[npairs], n1_all = off1[npairs];
  DGR_REQUIRE(n0_all < INT32_MAX && n1_all < INT32_MAX, "dgr_radius_pairs_batch: more than 2^31 rows");
  for (int i = 0; i < npairs * 16; ++i) DGR_REQUIRE(std::isfinite(T[i]), "dgr_radius_pairs_batch: non-finite pose");
  DGR_REQUIRE(capacity >= 0, "dgr_radius_pairs_batch: negative capacity");
  DGR_REQUIRE((xyz0 || n0_all == 0) && (xyz1 || n1_all == 0) && (counts_out || n0_all == 0),
              "dgr_radius_pairs_batch: NULL array");
  *total_out = 0;
  if (n0_all == 0) return DGR_OK;

  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  std::vector<GtPair> host(npairs);
  std::vector<DgrPointGrid> hgrids(npairs);
  int64_t max0 = 0;
  for (int p = 0; p < npairs; ++p) {
    GtPair &P = host[p];
    memset(&P, 0, sizeof(P));
    memcpy(P.T, T + (size_t)p * 16, 12 * sizeof(double));
    P.off0 = off0[p];
    P.n0 = (int32_t)(off0[p + 1] - off0[p]);
    max0 = std::max<int64_t>(max0, P.n0);
    memset(&hgrids[p], 0, sizeof(DgrPointGrid));
    hgrids[p].off = off1[p];
    hgrids[p].n = (int32_t)(off1[p + 1] - off1[p]);
  }
  GtPair *pairs;
  int64_t *total_pairs;
  DGR_ALLOC(pairs, A, GtPair, npairs);
  DGR_ALLOC(total_pairs, A, int64_t, 1);
  DGR_HIP_CHECK(hipMemcpyAsync(pairs, host.data(), (size_t)npairs * sizeof(GtPair), hipMemcpyHostToDevice, stream));
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64, &pin));
  volatile int64_t *landed = reinterpret_cast<volatile int64_t *>(pin);
  DgrPointGridSet grid;
  DGR_CHECK(dgr_point_grids_build(ctx, xyz1, hgrids.data(), npairs, radius, pin, "dgr_radius_pairs_batch", "batch", &grid, stream));
  const dim3 g0((unsigned)dgr_ceil_div(max0, GT_THREADS), npairs);
  const double r2 = radius * radius;
  gt_radius_kernel<false><<<g0, GT_THREADS, 0, stream>>>(xyz0, pairs, grid.grids, grid.cell_start, grid.sorted, r2, K, counts_out,
                                                        nullptr, nullptr);
  const int nsb = (int)dgr_ceil_div(n0_all, GT_SCAN_ROWS);
  int64_t *bsum, *row_off;
  DGR_ALLOC(bsum, A, int64_t, nsb);
  DGR_ALLOC(row_off, A, int64_t, n0_all + 1);
  gt_scan_sums_kernel<<<nsb, GT_THREADS, 0, stream>>>(counts_out, n0_all, bsum);
  gt_scan_blocks_kernel<<<1, GT_THREADS, 0, stream>>>(bsum, nsb, total_pairs);
  DGR_LAUNCH_CHECK();
  DGR_HIP_CHECK(hipMemcpyAsync(pin, total_pairs, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));
  const int64_t total = landed[0];
  *total_out = total;
  if (!pairs_out) return DGR_OK;
  DGR_REQUIRE(capacity >= total, "dgr_radius_pairs_batch: capacity %lld below the %lld pairs of the batch",
              (long long)capacity, (long long)total);
  gt_scan_final_kernel<<<nsb, GT_THREADS, 0, stream>>>(counts_out, n0_all, bsum, total_pairs, row_off);
  gt_radius_kernel<true><<<g0, GT_THREADS, 0, stream>>>(xyz0, pairs, grid.grids, grid.cell_start, grid.sorted, r2, K, nullptr,
                                                       row_off, reinterpret_cast<longlong2 *>(pairs_out));
  DGR_LAUNCH_CHECK();
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // like every entry point that returns host values, this one synchronises
  return DGR_OK;
}

// ================================================================================================
// pair membership: core/correspondence.py:14-53.  key = pair[:,0] + pair[:,1] * M in wrapping int64 (numpy's
// arithmetic, the reference's collisions under a small hash seed included); label = key of the predicted pair occurs among
// the keys of the positive pairs (np.isin).  One open-addressing set of 64-bit keys per pair of the batch, linear
// probing as in hash.h; the sets lie back to back in one table.
// ================================================================================================
constexpr unsigned long long GT_EMPTY = 0x8080808080808080ull;   // (hipMemsetAsync byte pattern)

struct GtSet {
  int64_t pos_off, pred_off;   // first row of the pair in pos / pred
  int64_t M;
  int64_t base;                // first slot of the pair's set
  uint64_t mask;               // slots - 1
};

__device__ __forceinline__ uint64_t gt_mix64(uint64_t x) {   // splitmix64 finaliser
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ int gt_segment(const GtSet *sets, int npairs, int64_t row, bool pred) {
  int lo = 0, hi = npairs - 1;   // last pair whose first row is <= row (empty pairs share a first row: the last wins)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((pred ? sets[mid].pred_off : sets[mid].pos_off) <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ unsigned long long gt_key(const int64_t *pair, int64_t M) {
  return (unsigned long long)pair[0] + (unsigned long long)pair[1] * (unsigned long long)M;
}

__global__ void __launch_bounds__(GT_THREADS)
    gt_set_insert_kernel(const int64_t *__restrict__ pos, int64_t n, const GtSet *__restrict__ sets, int npairs,
                         unsigned long long *table, int32_t *has_empty_key) {
  const int64_t r = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (r >= n) return;
  const int p = gt_segment(sets, npairs, r, false);
  const GtSet S = sets[p];
  const unsigned long long key = gt_key(pos + r * 2, S.M);
  if (key == GT_EMPTY) { has_empty_key[p] = 1; return; }   // the one key the table cannot hold
  uint64_t slot = gt_mix64(key) & S.mask;
  while (true) {
    const unsigned long long old = atomicCAS(&table[S.base + slot], GT_EMPTY, key);
    if (old == GT_EMPTY || old == key) return;
    slot = (slot + 1) & S.mask;
  }
}

__global__ void __launch_bounds__(GT_THREADS)
    gt_set_lookup_kernel(const int64_t *__restrict__ pred, int64_t n, const GtSet *__restrict__ sets, int npairs,
                         const unsigned long long *__restrict__ table, const int32_t *__restrict__ has_empty_key,
                         uint8_t *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (r >= n) return;
  const int p = gt_segment(sets, npairs, r, true);
  const GtSet S = sets[p];
  const unsigned long long key = gt_key(pred + r * 2, S.M);
  uint8_t hit = 0;
  if (key == GT_EMPTY) {
    hit = has_empty_key[p] ? 1 : 0;
  } else {
    uint64_t slot = gt_mix64(key) & S.mask;
    while (true) {   // ends: at most half of a set's slots are taken
      const unsigned long long v = table[S.base + slot];
      if (v == key) { hit = 1; break; }
      if (v == GT_EMPTY) break;
      slot = (slot + 1) & S.mask;
    }
  }
  out[r] = hit;
}

extern "C" int dgr_pairs_isin_batch(dgr_ctx *ctx, const int64_t *pos, const int64_t *pos_off, const int64_t *pred,
                                    const int64_t *pred_off, int npairs, const int64_t *M_per_pair, uint8_t *out,
                                    dgr_stream stream_) {
  DGR_REQUIRE(ctx && pos_off && pred_off && M_per_pair, "dgr_pairs_isin_batch: NULL argument");
  DGR_REQUIRE(npairs >= 1, "dgr_pairs_isin_batch: npairs = %d", npairs);
  DGR_REQUIRE(gt_offsets_ok(pos_off, npairs) && gt_offsets_ok(pred_off, npairs),
              "dgr_pairs_isin_batch: offsets must start at 0 and not decrease");
  const int64_t P = pos_off[npairs], Q = pred_off[npairs];
  DGR_REQUIRE((pos || P == 0) && ((pred && out) || Q == 0), "dgr_pairs_isin_batch: NULL array");
  if (Q == 0) return DGR_OK;
  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  std::vector<GtSet> host(npairs);
  int64_t slots = 0;
  for (int p = 0; p < npairs; ++p) {
    const int64_t np = pos_off[p + 1] - pos_off[p];
    const uint64_t cap = dgr_table_slots(np, 1ull << 62);
    host[p] = GtSet{pos_off[p], pred_off[p], M_per_pair[p], slots, cap - 1};
    slots += (int64_t)cap;
  }
  GtSet *sets;
  unsigned long long *table;
  int32_t *has_empty_key;
  DGR_ALLOC(sets, A, GtSet, npairs);
  DGR_ALLOC(table, A, unsigned long long, slots);
  DGR_ALLOC(has_empty_key, A, int32_t, npairs);
  DGR_HIP_CHECK(hipMemcpyAsync(sets, host.data(), (size_t)npairs * sizeof(GtSet), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemsetAsync(table, 0x80, (size_t)slots * sizeof(unsigned long long), stream));
  DGR_HIP_CHECK(hipMemsetAsync(has_empty_key, 0, (size_t)npairs * sizeof(int32_t), stream));
  if (P > 0)
    gt_set_insert_kernel<<<(unsigned)dgr_ceil_div(P, GT_THREADS), GT_THREADS, 0, stream>>>(pos, P, sets, npairs, table, has_empty_key);
  gt_set_lookup_kernel<<<(unsigned)dgr_ceil_div(Q, GT_THREADS), GT_THREADS, 0, stream>>>(pred, Q, sets, npairs, table, has_empty_key, out);
  DGR_LAUNCH_CHECK();
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // `host` and the arena are free again when this returns
  return DGR_OK;
}

// ================================================================================================
// validation counts: core/trainer.py:395, 430-437.  pred = weight > threshold; per pair (n, hits, tp, fp, tn, fn).
// Integers only: per-thread counts, a fixed-order wave and block reduction, one integer add per block and counter --
// exact in any order, so two runs agree bit for bit.
// ================================================================================================
constexpr int GT_COUNT_ROWS = 4096;   // rows per block

__global__ void __launch_bounds__(GT_THREADS)
    gt_counts_kernel(const uint8_t *__restrict__ label, const float *__restrict__ weights, float threshold,
                     const int64_t *__restrict__ off, unsigned long long *__restrict__ counts) {
  __shared__ int32_t red[GT_THREADS / 64][4];
  const int p = blockIdx.y;
  const int64_t lo = off[p] + (int64_t)blockIdx.x * GT_COUNT_ROWS, hi = min(off[p + 1], lo + GT_COUNT_ROWS);
  if (lo >= hi) return;   // block-uniform
  int32_t c[4] = {0, 0, 0, 0};   // tp, fp, tn, fn
  for (int64_t r = lo + threadIdx.x; r < hi; r += GT_THREADS) {
    const bool pos = label[r] != 0, pred = weights[r] > threshold;
    c[0] += pred && pos; c[1] += pred && !pos; c[2] += !pred && !pos; c[3] += !pred && pos;
  }
  for (int k = 0; k < 4; ++k) {
    int32_t v = c[k];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int32_t v = 0;
    for (int w = 0; w < GT_THREADS / 64; ++w) v += red[w][threadIdx.x];
    if (v) atomicAdd(&counts[p * 6 + 2 + threadIdx.x], (unsigned long long)v);
  }
}

extern "C" int dgr_validation_counts(dgr_ctx *ctx, const uint8_t *label, const float *weights, float threshold,
                                     const int64_t *off, int npairs, int64_t *counts_out, dgr_stream stream_) {
  DGR_REQUIRE(ctx && off && counts_out, "dgr_validation_counts: NULL argument");
  DGR_REQUIRE(npairs >= 1 && npairs <= GT_MAX_PAIRS, "dgr_validation_counts: npairs = %d (1..%d)", npairs, GT_MAX_PAIRS);
  DGR_REQUIRE(gt_offsets_ok(off, npairs), "dgr_validation_counts: offsets must start at 0 and not decrease");
  DGR_REQUIRE(!std::isnan(threshold), "dgr_validation_counts: threshold is NaN");
  const int64_t Q = off[npairs];
  DGR_REQUIRE((label && weights) || Q == 0, "dgr_validation_counts: NULL array");
  memset(counts_out, 0, (size_t)npairs * 6 * sizeof(int64_t));
  if (Q == 0) return DGR_OK;
  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  int64_t *off_dev, max_n = 0;
  unsigned long long *counts;
  DGR_ALLOC(off_dev, A, int64_t, npairs + 1);
  DGR_ALLOC(counts, A, unsigned long long, (size_t)npairs * 6);
  for (int p = 0; p < npairs; ++p) max_n = std::max(max_n, off[p + 1] - off[p]);
  DGR_HIP_CHECK(hipMemcpyAsync(off_dev, off, (size_t)(npairs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)npairs * 6 * sizeof(unsigned long long), stream));
  gt_counts_kernel<<<dim3((unsigned)dgr_ceil_div(max_n, GT_COUNT_ROWS), npairs), GT_THREADS, 0, stream>>>(label, weights, threshold,
                                                                                                       off_dev, counts);
  DGR_LAUNCH_CHECK();
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64 + (size_t)npairs * 6 * sizeof(int64_t), &pin));
  DGR_HIP_CHECK(hipMemcpyAsync(pin + 64, counts, (size_t)npairs * 6 * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));
  memcpy(counts_out, pin + 64, (size_t)npairs * 6 * sizeof(int64_t));
  for (int p = 0; p < npairs; ++p) {
    int64_t *c = counts_out + (size_t)p * 6;
    c[0] = off[p + 1] - off[p];   // n
    c[1] = c[2] + c[5];           // hits = tp + fn
  }
  return DGR_OK;
}
