// Feature-space k-nearest-neighbour search, 1 < k <= DGR_KNN_MAX_K, exact L2: core.knn.find_knn_gpu(..., knn=k) of the
// reference (core/knn.py:23-74), which repeats `min` k times over the full [chunk, N1] distance matrix.
//
// Every query keeps a sorted list of K packed keys (knn_key: D2 bits << 32 | row of the concatenated F1) in registers,
// K = k rounded up to a power of two.  D2 is knn_d2, the operation order of the 1-NN search, so column 0 is the 1-NN
// result bit for bit.  Only finite distances enter a list (the 1-NN kernels' `d < best` with best = inf).
//
// Brute force (every C): knn_topk_kernel, the tile loop of knn1_kernel with a list instead of a (min, argmin) pair.
// F1 is split over workgroups; a 64-bit atomicMin cannot merge lists, so every split writes its partial lists to
// scratch and knn_topk_merge combines them.
//
// Prefilter (C = 32, N1 >= KNN_MIN_REFS: knn_dispatch): the bf16-MFMA passes of knn_prefilter.h with a top-k bound.
//   pack     TOPK layout: the 32 SLOT CLASSES (rows sitting in slot s of some tile) are disjoint and each is spread
//            over the cloud.
//   pass 1   over a sample of the tiles (every SUB-th stage), the minimum of d~' per query and slot class: 32 minima,
//            attained by 32 distinct reference rows.  knn_topk_bound takes U = the k-th smallest of them.
//   pass 2   every (i, j) with d~'(i, j) <= U_j + tau_j goes to the query's candidate list (slots: 16 K).
//   exact    one thread per query re-evaluates its candidates exactly and keeps the K smallest keys.
// Why the list holds the exact top k: k distinct rows r_1 .. r_k have d~'(r_m) <= U -- pass 2 recomputes d~' with the
// instructions of pass 1 (one kernel template), so it sees the very values U was taken from.  The split error gives
// |d~'(r) + na_j - D2(r)| <= tau_j / 2 for every row r, so
// D2(r_m) <= U + na_j + tau_j / 2 and the k-th smallest exact D2 satisfies D2_(k) <= U + na_j + tau_j / 2.  Every row of
// the exact top k -- ties at D2_(k) under the index order included -- has D2(r) <= D2_(k), hence
// d~'(r) <= D2(r) - na_j + tau_j / 2 <= U + tau_j, and is emitted by pass 2.  The candidate list is therefore a superset
// of the exact top k and the exact pass returns the brute-force keys bit for bit.
// Fallbacks, no host round trip: a query with more candidates than slots is redone by knn_topk_scan_kernel (one
// workgroup per query, exact); a pair with non-finite / huge input, or with more than KNN_TOPK_SCAN_MAX such queries, is
// redone whole by the brute-force kernel behind (run flag per pair).
#include "knn_prefilter.h"

constexpr int KNN_TOPK_SCAN_MAX = 256;   // overflowing queries per pair redone one workgroup each; more: the pair by brute force
constexpr int KNN_TOPK_MAX_SPLITS = 16;  // F1 splits of the brute-force kernel (scratch: splits x N0 x k keys)

// slots per query and pass-1 sampling step of the prefilter for a list of K.  Expected candidates on iid ranks: about
// 2 x 32 (H_32 - H_(32-k)) with every 2nd stage sampled (k = 8: ~18, k = 16: ~43); k = 32 takes the max of the 32
// class minima (~32 H_32 = 130 with every stage sampled), hence its full first pass.
constexpr int knn_topk_slots(int K) { return K >= 32 ? 512 : 16 * K; }
constexpr int knn_topk_sub(int K) { return K >= 32 ? 1 : 2; }
// queries per thread of the brute-force kernel: query values + list within ~160 VGPRs
constexpr int knn_topk_qpt(int C, int K) { return (C + 2 * K) * 4 <= 160 ? 4 : ((C + 2 * K) * 2 <= 160 ? 2 : 1); }

// sorted insertion into the ascending register list L; the largest key drops out.  Keys are unique (the index part).
template <int K>
__device__ __forceinline__ void topk_insert(u64 (&L)[K], u64 key) {
  if (key < L[K - 1]) {
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
      const u64 lo = L[i - 1], cur = L[i];
      L[i] = lo > key ? lo : (cur < key ? cur : key);   // max(L[i-1], min(L[i], key))
    }
    L[0] = L[0] < key ? L[0] : key;
  }
}

// ------------------------------------------------------------------------------------------
// brute force.  Grid: x = query blocks (of the largest pair), y = F1 splits, z = pair.  part[(split * span + q -
// q_begin) * k + m] = m-th key of query row q (of the concatenated F0) over the split's references; a split without
// references writes empty lists.  run_flag (nullable): pairs whose flag is 0 are skipped.
// ------------------------------------------------------------------------------------------
template <int C, int K, int QPT>
__global__ void __launch_bounds__(KNN_THREADS)
    knn_topk_kernel(const float *__restrict__ F0, const float *__restrict__ F1, KnnBatch B, int splits, int k,
                    int64_t q_begin, int64_t span, u64 *__restrict__ part, const int32_t *__restrict__ run_flag) {
  __shared__ __attribute__((aligned(16))) float tile[KNN_TB * C];
  const KnnPair d = B.p[blockIdx.z];
  if (run_flag && run_flag[blockIdx.z] == 0) return;
  const int64_t N0 = d.n0, N1 = d.n1;
  if ((int64_t)blockIdx.x * KNN_THREADS * QPT >= N0) return;
  const int64_t ql0 = ((int64_t)blockIdx.x * KNN_THREADS + threadIdx.x) * QPT;   // pair-local query row
  const int rows_per_split = (int)(((N1 + splits - 1) / splits + KNN_TB - 1) / KNN_TB) * KNN_TB;
  const int64_t j_begin = (int64_t)blockIdx.y * rows_per_split;
  const int64_t j_end = min(N1, j_begin + rows_per_split);
  const float *F0p = F0 + d.q0 * C, *F1p = F1 + d.r0 * C;
  float q[QPT][C];
#pragma unroll
  for (int u = 0; u < QPT; ++u)
    knn_load_row<C>(q[u], F0p + min(ql0 + u, N0 - 1) * C);
  u64 L[QPT][K];
#pragma unroll
  for (int u = 0; u < QPT; ++u)
#pragma unroll
    for (int m = 0; m < K; ++m) L[u][m] = KNN_KEY_NONE;

  for (int64_t j0 = j_begin; j0 < j_end; j0 += KNN_TB) {   // block-uniform bounds
    const int nrows = (int)min((int64_t)KNN_TB, j_end - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < KNN_TB * C / 4; e += KNN_THREADS) {
      const int row = e / (C / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < nrows) v = *reinterpret_cast<const float4 *>(F1p + (j0 + row) * C + (e % (C / 4)) * 4);
      *reinterpret_cast<float4 *>(tile + e * 4) = v;
    }
    __syncthreads();
    for (int jj = 0; jj < nrows; ++jj) {
      const int64_t ridx = j0 + jj + d.r0;   // row of the concatenated F1
#pragma unroll
      for (int u = 0; u < QPT; ++u) {
        const float dd = knn_d2<C>(q[u], tile + jj * C);   // LDS broadcast
        if (dd < __builtin_inff()) topk_insert<K>(L[u], knn_key(dd, ridx));
      }
    }
  }
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    if (ql0 + u >= N0) continue;
    u64 *dst = part + ((int64_t)blockIdx.y * span + d.q0 + ql0 + u - q_begin) * k;
#pragma unroll
    for (int m = 0; m < K; ++m)
      if (m < k) dst[m] = L[u][m];
  }
}

// one thread per query: the k smallest keys over the splits' lists -> keys[q * k ..] (q = row of the concatenated F0)
template <int K>
__global__ void __launch_bounds__(256)
    knn_topk_merge(const u64 *__restrict__ part, KnnBatch B, int splits, int k, int64_t q_begin, int64_t span,
                   const int32_t *__restrict__ run_flag, u64 *__restrict__ keys) {
  const KnnPair d = B.p[blockIdx.y];
  if (run_flag && run_flag[blockIdx.y] == 0) return;
  const int64_t ql = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ql >= d.n0) return;
  const int64_t q = d.q0 + ql;
  u64 L[K];
#pragma unroll
  for (int m = 0; m < K; ++m) L[m] = KNN_KEY_NONE;
  for (int s = 0; s < splits; ++s) {
    const u64 *src = part + ((int64_t)s * span + q - q_begin) * k;
    for (int m = 0; m < k; ++m) {
      const u64 key = src[m];
      if (!(key < L[K - 1])) break;   // the split's list is sorted: nothing further of it enters
      topk_insert<K>(L, key);
    }
  }
#pragma unroll
  for (int m = 0; m < K; ++m)
    if (m < k) keys[q * k + m] = L[m];
}

// keys -> idx / dist, [n0, k] row-major.  Columns m >= n1: index 0 of the pair (its row r0 of the concatenated F1) and
// distance inf, what the reference's repeated min returns once the row is exhausted.  A column m < n1 without a key (a
// query with fewer finite distances) reads like the 1-NN kernels' empty result: index r0, the distance of key ~0.
__global__ void knn_topk_finish(const u64 *__restrict__ keys, KnnBatch B, int k, int squared,
                                int64_t *__restrict__ idx_out, float *__restrict__ dist_out) {
  const KnnPair d = B.p[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d.n0 * k) return;
  const int m = (int)(e % k);
  const int64_t i = d.q0 * k + e;
  const u64 key = keys[i];
  if (m >= d.n1) {
    idx_out[i] = d.r0;
    if (dist_out) dist_out[i] = __builtin_inff();
    return;
  }
  idx_out[i] = (key == KNN_KEY_NONE) ? d.r0 : (int64_t)(key & 0xffffffffull);
  if (dist_out) {
    const float d2 = __uint_as_float((unsigned int)(key >> 32));
    dist_out[i] = squared ? d2 : sqrtf(d2 + 1e-7f);   // pdist 'L2', core/metrics.py:64-65
  }
}

template <int C, int K>
static int knn_topk_brute(dgr_ctx *ctx, const float *F0, const float *F1, const KnnBatch &B, int k, u64 *keys,
                          const int32_t *run_flag, hipStream_t stream) {
  constexpr int QPT = knn_topk_qpt(C, K);
  int64_t q_begin;
  const int64_t span = knn_query_span(B, &q_begin);
  const dim3 grid = knn_brute_grid(ctx, B, QPT, KNN_TOPK_MAX_SPLITS);
  const int splits = (int)grid.y;
  u64 *part;
  DGR_ALLOC(part, ctx->arena, u64, (int64_t)splits * span * k);
  knn_topk_kernel<C, K, QPT><<<grid, KNN_THREADS, 0, stream>>>(F0, F1, B, splits, k, q_begin, span, part, run_flag);
  DGR_LAUNCH_CHECK();
  dim3 mgrid((unsigned)dgr_ceil_div(knn_n0_max(B), 256), B.np);
  knn_topk_merge<K><<<mgrid, 256, 0, stream>>>(part, B, splits, k, q_begin, span, run_flag, keys);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// ------------------------------------------------------------------------------------------
// prefilter (C = 32): what the top-k search adds to knn_prefilter.h.  Per-query scratch (KnnPlan) holds row q of the
// concatenated F0 at element q - q_begin.
// ------------------------------------------------------------------------------------------
// one thread per query: U = the k-th smallest of the 32 class minima pass 1 left in mt[s * span + q - q_begin],
// thr = U + tau (the tau of knn_prefilter.h)
__global__ void __launch_bounds__(256)
    knn_topk_bound(const uint32_t *__restrict__ mt, const float *__restrict__ nap, const uint32_t *__restrict__ nb_max,
                   KnnBatch B, int k, int64_t q_begin, int64_t span, float *__restrict__ thr_q) {
  const KnnPair d = B.p[blockIdx.y];
  const int64_t ql = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ql >= d.n0) return;
  const int64_t r = d.q0 - q_begin + ql;
  float v[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const float x = knn_unord(mt[(int64_t)s * span + r]);
    v[s] = (x == x) ? x : __builtin_inff();   // a class without a sampled row (cannot happen for n1 >= 1024): +inf
  }
  float U = __builtin_inff();
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    int rank = 0;
#pragma unroll
    for (int t = 0; t < 32; ++t) rank += (v[t] < v[s]) || (v[t] == v[s] && t < s);
    if (rank == k - 1) U = v[s];
  }
  const float nmax = __uint_as_float(nb_max[blockIdx.y]);
  thr_q[r] = U + KNN_TAU_C * (nap[(int64_t)d.qb0 * 32 + ql] + nmax);
}

// one thread per query row q in [q_begin, q_end): exact D2 of its candidates (rows of the concatenated F1), the K
// smallest keys -> keys[q * k ..].  Queries without candidates (pairs not in this batch) or with an overflowed list
// are left to the fallbacks.
template <int K>
__global__ void __launch_bounds__(256)
    knn_topk_exact_kernel(const float *__restrict__ F0, const float *__restrict__ F1, const int32_t *__restrict__ cand,
                          const int32_t *__restrict__ cand_cnt, int slots, int k, int64_t q_begin, int64_t q_end,
                          u64 *__restrict__ keys) {
  const int64_t q = q_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= q_end) return;
  const int cnt = cand_cnt[q - q_begin];
  if (cnt <= 0 || cnt > slots) return;
  float a[32];
  knn_load_row<32>(a, F0 + q * 32);
  u64 L[K];
#pragma unroll
  for (int m = 0; m < K; ++m) L[m] = KNN_KEY_NONE;
  const int32_t *cq = cand + (q - q_begin) * slots;
  for (int s = 0; s < cnt; ++s) {
    const int i = cq[s];
    const float dd = knn_d2<32>(a, F1 + (int64_t)i * 32);
    if (dd < __builtin_inff()) topk_insert<K>(L, knn_key(dd, i));
  }
#pragma unroll
  for (int m = 0; m < K; ++m)
    if (m < k) keys[q * k + m] = L[m];
}

// workgroup (x, pair) redoes the x-th listed query of the pair exactly: every thread keeps the K smallest keys of its
// strided share of the references, then k rounds of a workgroup minimum over the list heads pop the k smallest overall
// (a thread's list is the top K of its share: no thread can owe more than K of them).
template <int K>
__global__ void __launch_bounds__(256)
    knn_topk_scan_kernel(const float *__restrict__ F0, const float *__restrict__ F1, KnnBatch B, int k, int64_t q_begin,
                         const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount, u64 *__restrict__ keys) {
  __shared__ u64 wmin[2][4];
  const KnnPair d = B.p[blockIdx.y];
  const int n_q = qcount[blockIdx.y];
  if ((int)blockIdx.x >= n_q || n_q > KNN_TOPK_SCAN_MAX) return;   // block-uniform
  const int64_t q = d.q0 + qlist[d.q0 - q_begin + blockIdx.x];
  float a[32];
  knn_load_row<32>(a, F0 + q * 32);
  u64 L[K];
#pragma unroll
  for (int m = 0; m < K; ++m) L[m] = KNN_KEY_NONE;
  for (int j = (int)threadIdx.x; j < d.n1; j += 256) {
    const float dd = knn_d2<32>(a, F1 + (d.r0 + j) * 32);
    if (dd < __builtin_inff()) topk_insert<K>(L, knn_key(dd, j + d.r0));
  }
  for (int r = 0; r < k; ++r) {
    u64 mn = L[0];
#pragma unroll
    for (int s2 = 32; s2 > 0; s2 >>= 1) {
      const u64 o = __shfl_xor(mn, s2, 64);
      mn = o < mn ? o : mn;
    }
    if ((threadIdx.x & 63) == 0) wmin[r & 1][threadIdx.x >> 6] = mn;
    __syncthreads();   // (double buffer: round r + 2 writes this half only after every thread passed round r + 1's barrier)
    u64 g = wmin[r & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) g = wmin[r & 1][w] < g ? wmin[r & 1][w] : g;
    if (g != KNN_KEY_NONE && L[0] == g) {   // keys are unique: exactly one thread owns the minimum
#pragma unroll
      for (int m = 0; m < K - 1; ++m) L[m] = L[m + 1];
      L[K - 1] = KNN_KEY_NONE;
    }
    if (threadIdx.x == 0) keys[q * k + r] = g;
  }
}

// pairs redone whole by the brute-force kernel: non-finite / huge input, or more overflowing queries than the scan takes
__global__ void knn_topk_redo_flags(const int32_t *__restrict__ fallback, const int32_t *__restrict__ qcount, int np,
                                    int32_t *__restrict__ flags) {
  if ((int)threadIdx.x < np) flags[threadIdx.x] = fallback[threadIdx.x] != 0 || qcount[threadIdx.x] > KNN_TOPK_SCAN_MAX;
}

template <int K>
static int knn_topk_prefiltered(dgr_ctx *ctx, const float *F0, const float *F1, KnnBatch B, int k, u64 *keys,
                                hipStream_t stream) {
  constexpr int SLOTS = knn_topk_slots(K), SUB = knn_topk_sub(K);
  KnnPlan P;
  DGR_CHECK(knn_prefilter_setup<true>(ctx, F0, F1, B, SLOTS, stream, &P));
  DGR_CHECK((knn_mfma_launch<false, true>(ctx, B, P, SUB, SLOTS, stream)));
  dim3 grid((unsigned)dgr_ceil_div(P.n0_max, 256), B.np);
  knn_topk_bound<<<grid, 256, 0, stream>>>(P.mt, P.na, P.nb_max, B, k, P.q_begin, P.span, P.thr);
  DGR_LAUNCH_CHECK();
  DGR_CHECK((knn_mfma_launch<true, true>(ctx, B, P, 1, SLOTS, stream)));
  knn_topk_exact_kernel<K><<<(unsigned)dgr_ceil_div(P.span, 256), 256, 0, stream>>>(
      F0, F1, P.cand, P.cand_cnt, SLOTS, k, P.q_begin, P.q_begin + P.span, keys);
  DGR_LAUNCH_CHECK();
  DGR_CHECK(knn_list_overflows(B, P, SLOTS, stream));
  dim3 sgrid(KNN_TOPK_SCAN_MAX, B.np);   // normally (almost) empty: the workgroups beyond the list return at once
  knn_topk_scan_kernel<K><<<sgrid, 256, 0, stream>>>(F0, F1, B, k, P.q_begin, P.qlist, P.qcount, keys);
  knn_topk_redo_flags<<<1, 64, 0, stream>>>(P.fallback, P.qcount, B.np, P.flags);
  DGR_LAUNCH_CHECK();
  DGR_CHECK((knn_topk_brute<32, K>(ctx, F0, F1, B, k, keys, P.flags, stream)));
  return knn_trace_prefiltered(ctx, B, P, stream);
}

template <int K>
static int knn_topk_batch(dgr_ctx *ctx, const float *F0, const float *F1, const KnnBatch &B, int C, int k,
                          u64 *keys, hipStream_t stream) {
  return knn_dispatch(
      B, C,
      [&](auto width, const KnnBatch &pairs) {
        return knn_topk_brute<decltype(width)::value, K>(ctx, F0, F1, pairs, k, keys, nullptr, stream);
      },
      [&](const KnnBatch &pairs) { return knn_topk_prefiltered<K>(ctx, F0, F1, pairs, k, keys, stream); });
}

// pairs = row ranges off0 / off1 (host, starting at 0, none empty) of the concatenated F0 / F1; k in [2, DGR_KNN_MAX_K]
static int knn_topk_impl(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1, const int64_t *off1,
                         int npairs, int C, int k, int squared, int64_t *idx_out, float *dist_out, hipStream_t stream) {
  const int K = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32;
  return knn_for_each_table(ctx, off0, off1, npairs, k, false, stream, [&](const KnnBatch &B, u64 *keys) -> int {
    switch (K) {
      case 2: DGR_CHECK(knn_topk_batch<2>(ctx, F0, F1, B, C, k, keys, stream)); break;
      case 4: DGR_CHECK(knn_topk_batch<4>(ctx, F0, F1, B, C, k, keys, stream)); break;
      case 8: DGR_CHECK(knn_topk_batch<8>(ctx, F0, F1, B, C, k, keys, stream)); break;
      case 16: DGR_CHECK(knn_topk_batch<16>(ctx, F0, F1, B, C, k, keys, stream)); break;
      default: DGR_CHECK(knn_topk_batch<32>(ctx, F0, F1, B, C, k, keys, stream)); break;
    }
    dim3 grid((unsigned)dgr_ceil_div(knn_n0_max(B) * k, 256), B.np);
    knn_topk_finish<<<grid, 256, 0, stream>>>(keys, B, k, squared, idx_out, dist_out);
    DGR_LAUNCH_CHECK();
    return DGR_OK;
  });
}

extern "C" int dgr_knn_l2_batch(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1,
                                const int64_t *off1, int npairs, int C, int k, int squared, int64_t *idx_out,
                                float *dist_out, dgr_stream stream) {
  DGR_REQUIRE(k >= 1 && k <= DGR_KNN_MAX_K, "dgr_knn_l2_batch: k=%d outside [1, %d]", k, DGR_KNN_MAX_K);
  if (k == 1) return dgr_knn1_l2_batch(ctx, F0, off0, F1, off1, npairs, C, squared, idx_out, dist_out, stream);
  DGR_CHECK(knn_enter("dgr_knn_l2_batch", ctx, F0, F1, idx_out, off0, off1, npairs));
  return knn_topk_impl(ctx, F0, off0, F1, off1, npairs, C, k, squared, idx_out, dist_out, (hipStream_t)stream);
}

extern "C" int dgr_knn_l2(dgr_ctx *ctx, const float *F0, int64_t N0, const float *F1, int64_t N1, int C, int k,
                          int squared, int64_t *idx_out, float *dist_out, dgr_stream stream) {
  DGR_REQUIRE(k >= 1 && k <= DGR_KNN_MAX_K, "dgr_knn_l2: k=%d outside [1, %d]", k, DGR_KNN_MAX_K);
  if (k == 1) return dgr_knn1_l2(ctx, F0, N0, F1, N1, C, squared, idx_out, dist_out, stream);
  const int64_t off0[2] = {0, N0}, off1[2] = {0, N1};
  DGR_CHECK(knn_enter("dgr_knn_l2", ctx, F0, F1, idx_out, off0, off1, 1));
  return knn_topk_impl(ctx, F0, off0, F1, off1, 1, C, k, squared, idx_out, dist_out, (hipStream_t)stream);
}
