// Definitions shared by the feature-space k-NN searches, knn.hip (1-NN) and knn_topk.hip (top-k): the pair descriptor
// table, the exact distance and its key, and the host driver (argument checks, descriptor tables, small / large policy).
// The bf16-MFMA prefilter both searches run for C = 32 is knn_prefilter.h.
#pragma once
#include <type_traits>
#include "dgr_internal.h"

constexpr int KNN_THREADS = 256;
constexpr int KNN_TB = 64;  // F1 rows per LDS tile
constexpr int KNN_MAXP = 32;   // pairs per launch (descriptor table passed by value: no upload, no host buffer to keep alive)
constexpr int KNN_MIN_REFS = 1024;   // C = 32: pairs with fewer references go to the brute-force kernel alone

struct KnnPair {
  int64_t q0, r0;      // first query row (of F0) / first reference row (of F1) of the pair
  int32_t n0, n1;      // queries / references
  int32_t qb0, rt0;    // first 32-row block of the pair in the packed query / reference arrays
};
struct KnnBatch {
  KnnPair p[KNN_MAXP];
  int np;
};

// Packed result key (D2 bits << 32 | row of the concatenated F1): positive floats order like their bit patterns, so the
// keys order like (f32 D2, index) -- equal distances: the smaller index first, like torch.min on the CPU.
typedef unsigned long long u64;
constexpr u64 KNN_KEY_NONE = ~0ull;
__device__ __forceinline__ u64 knn_key(float d2, int64_t row) {
  return ((u64)__float_as_uint(d2) << 32) | (unsigned int)row;
}

// sum_c (a_c - b_c)^2 in the operation order that defines the result bits: two interleaved fma chains, then one add.
// (The definition is the inner loop of knn1_kernel, knn.hip, which shares one LDS read of b between its queries.)
template <int C>
__device__ __forceinline__ float knn_d2(const float (&a)[C], const float *__restrict__ b) {
  float d0 = 0.f, d1 = 0.f;
#pragma unroll
  for (int c = 0; c < C; c += 4) {
    const float4 bv = *reinterpret_cast<const float4 *>(b + c);
    const float e0 = a[c] - bv.x, e1 = a[c + 1] - bv.y, e2 = a[c + 2] - bv.z, e3 = a[c + 3] - bv.w;
    d0 = fmaf(e0, e0, d0);
    d1 = fmaf(e1, e1, d1);
    d0 = fmaf(e2, e2, d0);
    d1 = fmaf(e3, e3, d1);
  }
  return d0 + d1;
}

// the C-wide query row `src` into registers
template <int C>
__device__ __forceinline__ void knn_load_row(float (&a)[C], const float *__restrict__ src) {
#pragma unroll
  for (int c = 0; c < C; c += 4) {
    const float4 v = *reinterpret_cast<const float4 *>(src + c);
    a[c] = v.x; a[c + 1] = v.y; a[c + 2] = v.z; a[c + 3] = v.w;
  }
}

// ------------------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------------------
inline int64_t knn_n0_max(const KnnBatch &B) {
  int64_t n = 0;
  for (int p = 0; p < B.np; ++p) n = std::max<int64_t>(n, B.p[p].n0);
  return n;
}

// query rows SPANNED by the pairs of B in the concatenated F0 (not the sum of their rows), from row *q_begin on
inline int64_t knn_query_span(const KnnBatch &B, int64_t *q_begin) {
  int64_t q_end = 0;
  *q_begin = B.p[0].q0;
  for (int p = 0; p < B.np; ++p) {
    *q_begin = std::min(*q_begin, B.p[p].q0);
    q_end = std::max(q_end, B.p[p].q0 + B.p[p].n0);
  }
  return q_end - *q_begin;
}

// Grid of a brute-force kernel that keeps `qpt` queries per thread: x = query blocks (of the largest pair), y = F1
// splits, z = pair.  Enough (query block, split) workgroups to cover every CU a few times over; a pair with fewer rows
// than the largest leaves its surplus blocks / splits empty (they exit at once).
inline dim3 knn_brute_grid(const dgr_ctx *ctx, const KnnBatch &B, int qpt, int64_t max_splits) {
  int64_t n1_max = 0, qblocks_all = 0;
  for (int p = 0; p < B.np; ++p) {
    n1_max = std::max<int64_t>(n1_max, B.p[p].n1);
    qblocks_all += dgr_ceil_div(B.p[p].n0, (int64_t)KNN_THREADS * qpt);
  }
  int64_t splits = dgr_ceil_div((int64_t)ctx->num_cus * 4, qblocks_all);
  splits = std::max<int64_t>(1, std::min(splits, std::min(max_splits, dgr_ceil_div(n1_max, KNN_TB))));
  return dim3((unsigned)dgr_ceil_div(knn_n0_max(B), (int64_t)KNN_THREADS * qpt), (unsigned)splits, B.np);
}

// What the extern "C" entries check before they touch the device, then the arena reset every public call starts with.
// The single-pair entries pass their N0 / N1 as two-element offset arrays.
inline int knn_enter(const char *entry, dgr_ctx *ctx, const void *F0, const void *F1, const void *idx_out,
                     const int64_t *off0, const int64_t *off1, int npairs) {
  DGR_REQUIRE(ctx && F0 && F1 && off0 && off1 && idx_out, "%s: NULL argument", entry);
  DGR_REQUIRE(npairs >= 1, "%s: npairs=%d", entry, npairs);
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  return ctx->arena.reset();
}

// Opt-in route trace (dgr_ctx_set_knn_trace, read back by dgr_debug_knn_trace; a test instrument).  One row of
// DGR_KNN_TRACE_FIELDS = 8 words per pair of the last call: {pair of the call, table, route (0 brute force / 1 prefiltered),
// fallback flag, overflow list length, redo-by-brute-force flag, largest cand_cnt, queries with cand_cnt == 0}.
// knn_trace_table opens the rows of a table, all on route 0; knn_trace_prefiltered (knn_prefilter.h) fills in the pairs
// of its prefiltered sub-batch.  With the trace off neither runs: a call issues the launches and copies it always did.
inline void knn_trace_table(dgr_ctx *ctx, const KnnBatch &B, int p0) {
  if (p0 == 0) ctx->knn_trace_rows.clear();
  ctx->knn_trace_q0.clear();
  for (int p = 0; p < B.np; ++p) {
    const int32_t row[DGR_KNN_TRACE_FIELDS] = {p0 + p, p0 / KNN_MAXP, 0, 0, 0, 0, 0, 0};
    ctx->knn_trace_rows.insert(ctx->knn_trace_rows.end(), row, row + DGR_KNN_TRACE_FIELDS);
    ctx->knn_trace_q0.push_back(B.p[p].q0);
  }
}

// Pairs = row ranges off0 / off1 (host arrays) of the concatenated F0 / F1.  Allocates the result keys (k per query row;
// `clear`: set to KNN_KEY_NONE, for a search that merges into them), cuts the pairs into descriptor tables of KNN_MAXP
// and runs fn(table, keys) for each, its scratch taken from the arena and given back afterwards.
template <class Fn>
inline int knn_for_each_table(dgr_ctx *ctx, const int64_t *off0, const int64_t *off1, int npairs, int k, bool clear,
                              hipStream_t stream, Fn &&fn) {
  const int64_t n0 = off0[npairs];
  DGR_REQUIRE(off0[0] == 0 && off1[0] == 0, "find_knn: the row offsets start at 0");
  DGR_REQUIRE(off1[npairs] < (1ll << 31) && n0 < (1ll << 31), "find_knn: N0 / N1 too large");
  u64 *keys;
  DGR_ALLOC(keys, ctx->arena, u64, n0 * k);
  if (clear) DGR_HIP_CHECK(hipMemsetAsync(keys, 0xff, (size_t)(n0 * k) * sizeof(u64), stream));
  for (int p0 = 0; p0 < npairs; p0 += KNN_MAXP) {
    KnnBatch B;
    B.np = std::min(KNN_MAXP, npairs - p0);
    for (int p = 0; p < B.np; ++p) {
      KnnPair &d = B.p[p];
      d.q0 = off0[p0 + p]; d.r0 = off1[p0 + p];
      d.n0 = (int32_t)(off0[p0 + p + 1] - off0[p0 + p]); d.n1 = (int32_t)(off1[p0 + p + 1] - off1[p0 + p]);
      d.qb0 = d.rt0 = 0;
      DGR_REQUIRE(d.n0 > 0 && d.n1 > 0, "find_knn: pair %d has an empty feature matrix (N0=%d, N1=%d)", p0 + p, d.n0,
                  d.n1);
    }
    const DgrArena::Mark mk = ctx->arena.mark();
    if (ctx->knn_trace) knn_trace_table(ctx, B, p0);
    DGR_CHECK(fn(B, keys));
    ctx->arena.rewind(mk);
  }
  return DGR_OK;
}

// Which kernels search the pairs of B: brute(width, pairs) for C = 16 / 64, for pairs with small reference sets (the
// prefilter's fixed passes would cost more) and for everything under DGR_KNN_BRUTE; prefiltered(pairs) for the rest.
// `width` is a std::integral_constant: the callables are generic lambdas that instantiate their kernels with it.
inline bool knn_force_brute() {
  static const bool brute = getenv("DGR_KNN_BRUTE") != nullptr;
  return brute;
}
template <class Brute, class Prefiltered>
inline int knn_dispatch(const KnnBatch &B, int C, Brute &&brute, Prefiltered &&prefiltered) {
  switch (C) {
    case 16: return brute(std::integral_constant<int, 16>{}, B);
    case 64: return brute(std::integral_constant<int, 64>{}, B);
    case 32: {
      KnnBatch big, small;
      big.np = small.np = 0;
      for (int p = 0; p < B.np; ++p) {
        if (knn_force_brute() || B.p[p].n1 < KNN_MIN_REFS) small.p[small.np++] = B.p[p];
        else big.p[big.np++] = B.p[p];
      }
      if (small.np) DGR_CHECK(brute(std::integral_constant<int, 32>{}, small));
      if (big.np) DGR_CHECK(prefiltered(big));
      return DGR_OK;
    }
    default:
      dgr_set_error("find_knn: feature width %d not supported (16, 32, 64)", C);
      return DGR_EINVAL;
  }
}
