// Averaging voxel down-sample (Open3D's voxel_down_sample, the reference's util/pointcloud.py:72-80 preprocessing) of the
// selected fragments of a bank, each under its own rigid pose: every occupied voxel of ONE lattice is replaced by the mean
// of the points that fall into it.  One fragment without a pose is the down-sample of a cloud; all fragments of a scene
// under their optimised poses are the fused scene.  include/dgr_hip.h at dgr_voxel_mean states the arithmetic in full.
//
// Passes (one thread per selected row unless noted; rows are numbered in ascending row of `xyz`):
//   vm_quantise    pose, u = (p - origin) / voxel, c = floor(u), k = floor((u - c) 2^40); dropped rows are counted
//   unique rows    dgr_unique_rows over the 3-int keys, dropped rows skipped: the row's voxel = the smallest row of its key
//                  (kept in row_first), flag = "I am that row", rank of a voxel = first-occurrence order; a call of its own
//                  behind vm_quantise, so that every key it compares against was written by a finished kernel
//   vm_clear       zeroes count and sums of the V voxels (V is known on the device only)
//   vm_accumulate  no-return integer atomics: count += 1 (int32), sums += k (3 x uint64); first rows write first / coords
//   vm_finalise    one thread per voxel: mean = origin + (c + S / (n 2^40)) voxel
//
// Determinism: every per-row value is a function of the row alone and integer addition is associative and commutative,
// so the order in which the atomics are served does not reach the result -- no floating-point atomics anywhere.
#include "dgr_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

constexpr int VM_THREADS = 256;
constexpr double VM_FRAC_SCALE = (double)(1ull << DGR_VM_FRAC_BITS);

// one selected fragment, in ascending fragment order
struct VmSeg {
  double T[12];      // [R | t] row-major 3x4 (unused without poses)
  int64_t xyz_off;   // first row of the fragment in xyz
  int64_t sel_base;  // first of its rows in the call's row numbering
};

struct VmLattice {
  double origin[3], voxel;
};

// the segment of selected row r: the last one that starts at or before it (nseg >= 1, base[0] = 0)
__device__ __forceinline__ int vm_segment_of(const int64_t *__restrict__ base, int nseg, int64_t r) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename T>
__global__ void __launch_bounds__(VM_THREADS)
    vm_quantise(const T *__restrict__ xyz, const VmSeg *__restrict__ segs, const int64_t *__restrict__ seg_base, int nseg,
                int has_T, VmLattice L, int64_t n, int32_t *__restrict__ keys, unsigned long long *__restrict__ frac,
                int32_t *__restrict__ row_first, int32_t *dropped) {
#pragma clang fp contract(off)   // the pose and the lattice arithmetic are DEFINED without fma (include/dgr_hip.h)
  const int64_t r = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x;
  bool drop = false;
  if (r < n) {
    const VmSeg *S = segs + vm_segment_of(seg_base, nseg, r);
    const T *s = xyz + (S->xyz_off + (r - S->sel_base)) * 3;
    const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
    double p[3] = {x, y, z};
    if (has_T) {
      p[0] = ((S->T[0] * x + S->T[1] * y) + S->T[2] * z) + S->T[3];
      p[1] = ((S->T[4] * x + S->T[5] * y) + S->T[6] * z) + S->T[7];
      p[2] = ((S->T[8] * x + S->T[9] * y) + S->T[10] * z) + S->T[11];
    }
    int32_t c[3];
    unsigned long long k[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double u = (p[d] - L.origin[d]) / L.voxel;
      if (!(u >= -2147483648.0 && u < 2147483648.0)) drop = true;   // (a NaN fails both comparisons, an infinity one)
      const double f = floor(u);
      c[d] = drop ? 0 : (int32_t)f;
      k[d] = drop ? 0ull : (unsigned long long)floor((u - f) * VM_FRAC_SCALE);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      keys[r * 3 + d] = c[d];
      frac[r * 3 + d] = k[d];
    }
    row_first[r] = drop ? DGR_ROW_DROPPED : DGR_ROW_PENDING;
  }
  const unsigned long long b = __ballot(drop);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(dropped, __popcll(b));
}

__global__ void __launch_bounds__(VM_THREADS)
    vm_clear(const int32_t *__restrict__ n_dev, int32_t *__restrict__ count, unsigned long long *__restrict__ sums) {
  const int64_t v = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x;
  if (v >= *n_dev) return;
  count[v] = 0;
  sums[v * 3] = sums[v * 3 + 1] = sums[v * 3 + 2] = 0ull;
}

__global__ void __launch_bounds__(VM_THREADS)
    vm_accumulate(const int32_t *__restrict__ keys, const unsigned long long *__restrict__ frac,
                  const int32_t *__restrict__ row_first, const int32_t *__restrict__ rank, const VmSeg *__restrict__ segs,
                  const int64_t *__restrict__ seg_base, int nseg, int64_t n, int64_t *__restrict__ first_out,
                  int32_t *__restrict__ coords_out, int32_t *count, unsigned long long *sums) {
  const int64_t r = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x;
  if (r >= n) return;
  const int32_t fr = row_first[r];
  if (fr < 0) return;
  const int64_t v = rank[fr];
  atomicAdd(&count[v], 1);   // (results unused: no-return atomics)
#pragma unroll
  for (int d = 0; d < 3; ++d) atomicAdd(&sums[v * 3 + d], frac[r * 3 + d]);
  if (fr == (int32_t)r) {
    const VmSeg *S = segs + vm_segment_of(seg_base, nseg, r);
    first_out[v] = S->xyz_off + (r - S->sel_base);
#pragma unroll
    for (int d = 0; d < 3; ++d) coords_out[v * 3 + d] = keys[r * 3 + d];
  }
}

__global__ void __launch_bounds__(VM_THREADS)
    vm_finalise(const int32_t *__restrict__ n_dev, const int32_t *__restrict__ coords, const int32_t *__restrict__ count,
                const unsigned long long *__restrict__ sums, VmLattice L, double *__restrict__ mean) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x;
  if (v >= *n_dev) return;
  const double den = (double)count[v] * VM_FRAC_SCALE;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double s = (double)(long long)sums[v * 3 + d];
    mean[v * 3 + d] = L.origin[d] + ((double)coords[v * 3 + d] + s / den) * L.voxel;
  }
}

extern "C" int dgr_voxel_mean(dgr_ctx *ctx, const void *xyz, int is_f64, const int64_t *off, int nfrag,
                              const int32_t *frag_ids, int nsel, const double *T, const double *origin, double voxel_size,
                              int64_t *first_out, int32_t *coords_out, int32_t *count_out, int64_t *fsum_out,
                              double *mean_out, int64_t *n_out, int64_t *dropped_out, dgr_stream stream_) {
  // argument errors first: nothing has touched the device when one of them is reported
  DGR_REQUIRE(ctx && xyz && off && origin && first_out && coords_out && count_out && mean_out && n_out && dropped_out,
              "dgr_voxel_mean: NULL argument");
  DGR_REQUIRE(nfrag >= 1, "dgr_voxel_mean: nfrag = %d", nfrag);
  DGR_REQUIRE(nsel >= 1, "dgr_voxel_mean: nsel = %d", nsel);
  DGR_REQUIRE(frag_ids || nsel == nfrag, "dgr_voxel_mean: without frag_ids nsel must be nfrag (%d), got %d", nfrag, nsel);
  DGR_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "dgr_voxel_mean: voxel_size must be positive and finite");
  for (int d = 0; d < 3; ++d) DGR_REQUIRE(std::isfinite(origin[d]), "dgr_voxel_mean: non-finite origin");
  DGR_REQUIRE(off[0] >= 0, "dgr_voxel_mean: off[0] = %lld", (long long)off[0]);
  for (int f = 0; f < nfrag; ++f)
    DGR_REQUIRE(off[f + 1] > off[f], "dgr_voxel_mean: fragment %d of the bank is empty", f);
  // the selected fragments in ascending fragment order (order[k] = position in frag_ids): rows are numbered by their row
  // in xyz, so the result does not depend on the order of frag_ids
  std::vector<int> order(nsel);
  std::iota(order.begin(), order.end(), 0);
  if (frag_ids) {
    std::vector<char> seen(nfrag, 0);
    for (int k = 0; k < nsel; ++k) {
      DGR_REQUIRE(frag_ids[k] >= 0 && frag_ids[k] < nfrag, "dgr_voxel_mean: fragment id %d outside [0, %d)", frag_ids[k], nfrag);
      DGR_REQUIRE(!seen[frag_ids[k]], "dgr_voxel_mean: fragment id %d is repeated", frag_ids[k]);
      seen[frag_ids[k]] = 1;
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return frag_ids[a] < frag_ids[b]; });
  }
  if (T)
    for (int k = 0; k < nsel; ++k)
      for (int e = 0; e < 12; ++e)
        DGR_REQUIRE(std::isfinite(T[(size_t)k * 16 + e]), "dgr_voxel_mean: pose %d is not finite", k);
  std::vector<VmSeg> hsegs(nsel);
  std::vector<int64_t> hbase(nsel);
  int64_t n = 0;
  for (int s = 0; s < nsel; ++s) {
    const int k = order[s], f = frag_ids ? frag_ids[k] : k;
    VmSeg &S = hsegs[s];
    memset(&S, 0, sizeof(S));
    if (T) memcpy(S.T, T + (size_t)k * 16, 12 * sizeof(double));
    S.xyz_off = off[f];
    S.sel_base = hbase[s] = n;
    n += off[f + 1] - off[f];
    DGR_REQUIRE(n < (1ll << 31), "dgr_voxel_mean: 2^31 or more selected rows");
  }

  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  // pinned host memory of the context: [0, 64) the two int32 counters the call ends with, then the fragment records and
  // their first rows, uploaded from there -- the context's buffer outlives every path out of this function, the early
  // returns of a failed launch included, which the vectors above would not
  const size_t seg_bytes = (size_t)nsel * sizeof(VmSeg), base_bytes = (size_t)nsel * sizeof(int64_t);
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64 + seg_bytes + base_bytes, &pin));
  memcpy(pin + 64, hsegs.data(), seg_bytes);
  memcpy(pin + 64 + seg_bytes, hbase.data(), base_bytes);
  VmSeg *segs;
  int64_t *seg_base;
  int32_t *keys, *row_first, *flag, *rank, *counters;   // counters[0] = voxels, [1] = dropped rows
  unsigned long long *frac, *sums = reinterpret_cast<unsigned long long *>(fsum_out);
  DGR_ALLOC(segs, A, VmSeg, nsel);
  DGR_ALLOC(seg_base, A, int64_t, nsel);
  DGR_ALLOC(keys, A, int32_t, n * 3);
  DGR_ALLOC(frac, A, unsigned long long, n * 3);
  DGR_ALLOC(row_first, A, int32_t, n);
  DGR_ALLOC(flag, A, int32_t, n);
  DGR_ALLOC(rank, A, int32_t, n);
  DGR_ALLOC(counters, A, int32_t, 2);
  if (!sums) DGR_ALLOC(sums, A, unsigned long long, n * 3);
  DGR_HIP_CHECK(hipMemcpyAsync(segs, pin + 64, seg_bytes, hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(seg_base, pin + 64 + seg_bytes, base_bytes, hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), stream));
  VmLattice L;
  for (int d = 0; d < 3; ++d) L.origin[d] = origin[d];
  L.voxel = voxel_size;
  const unsigned grid = (unsigned)dgr_ceil_div(n, VM_THREADS);
  if (is_f64)
    vm_quantise<double><<<grid, VM_THREADS, 0, stream>>>((const double *)xyz, segs, seg_base, nsel, T != nullptr, L, n, keys, frac,
                                                         row_first, counters + 1);
  else
    vm_quantise<float><<<grid, VM_THREADS, 0, stream>>>((const float *)xyz, segs, seg_base, nsel, T != nullptr, L, n, keys, frac,
                                                        row_first, counters + 1);
  DGR_LAUNCH_CHECK();
  int32_t *table;   // (the key hash: not read again here)
  uint32_t mask;
  DGR_CHECK(dgr_unique_rows(A, keys, n, 3, row_first, row_first, flag, rank, counters, &table, &mask, stream));
  vm_clear<<<grid, VM_THREADS, 0, stream>>>(counters, count_out, sums);
  vm_accumulate<<<grid, VM_THREADS, 0, stream>>>(keys, frac, row_first, rank, segs, seg_base, nsel, n, first_out, coords_out,
                                                 count_out, sums);
  vm_finalise<<<grid, VM_THREADS, 0, stream>>>(counters, coords_out, count_out, sums, L, mean_out);
  DGR_LAUNCH_CHECK();
  DGR_HIP_CHECK(hipMemcpyAsync(pin, counters, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // like every entry point that returns host values, this one synchronises
  int32_t res[2];
  memcpy(res, pin, sizeof(res));
  *n_out = res[0];
  *dropped_out = res[1];
  return DGR_OK;
}
