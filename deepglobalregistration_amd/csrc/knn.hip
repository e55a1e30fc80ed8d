// Feature-space 1-nearest-neighbour search, exact L2, brute force.
// Replaces core.knn.find_knn_gpu (core/knn.py:23-74) + core.metrics.pdist (core/metrics.py:62-69).
//
// The reference materialises a [250, N1, 32] difference tensor per chunk (82 GB written and
// re-read per 26k x 24k pair).  Here nothing is materialised: a workgroup keeps QPT queries per
// thread in registers, streams tiles of F1 through LDS (broadcast ds_read_b128), evaluates the
// exact sum_c (a_c - b_c)^2 form in f32 on the vector ALUs (so the arg-min agrees with `pdist`
// instead of the cancellation-prone |a|^2+|b|^2-2ab expansion), keeps a running (min, argmin) per
// query, and merges the partial results of the F1 splits with one 64-bit atomicMin per query on
// the packed key (dist_bits << 32 | index): positive floats order like their bit patterns, and
// ties resolve to the smallest index like torch.min on the CPU.
//
// Batched (round 5): every kernel below runs ONCE for all pairs of a batch -- blockIdx.z (packing: blockIdx.y) selects
// the pair, whose row ranges inside the concatenated feature matrices come from a by-value descriptor table -- instead
// of 13 launches per pair in a host loop; reference indices are written as rows of the concatenated F1.
#include "knn_prefilter.h"

template <int C, int QPT>
__global__ void __launch_bounds__(KNN_THREADS)
    knn1_kernel(const float *__restrict__ F0, const float *__restrict__ F1, KnnBatch B, int splits,
                u64 *__restrict__ best, const int32_t *run_flag, const int32_t *__restrict__ qlist,
                const int32_t *qcount, int64_t q_begin) {
  __shared__ __attribute__((aligned(16))) float tile[KNN_TB * C];
  // blockIdx.z = pair: its rows of F0 / F1 / best (and of qlist), its flag and its list length
  const KnnPair d = B.p[blockIdx.z];
  if (run_flag && run_flag[blockIdx.z] == 0) return;  // fallback launch of the prefiltered path: nothing to redo
  F0 += d.q0 * C;
  F1 += d.r0 * C;
  best += d.q0;
  const int64_t N0 = d.n0, N1 = d.n1;
  // optional indirection: only the pair's queries listed in qlist[q0 - q_begin ..], qcount[pair] of them (prefilter
  // slot overflow; q_begin: the first query row the list array covers)
  if (qlist) qlist += d.q0 - q_begin;
  const int64_t n_q = qlist ? (int64_t)qcount[blockIdx.z] : N0;
  if ((int64_t)blockIdx.x * KNN_THREADS * QPT >= n_q) return;
  const int64_t q0 = ((int64_t)blockIdx.x * KNN_THREADS + threadIdx.x) * QPT;
  const int rows_per_split = (int)(((N1 + splits - 1) / splits + KNN_TB - 1) / KNN_TB) * KNN_TB;
  const int64_t j_begin = (int64_t)blockIdx.y * rows_per_split;
  const int64_t j_end = min(N1, j_begin + rows_per_split);
  if (j_begin >= j_end) return;
  float q[QPT][C];
  int64_t qrow[QPT];
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const int64_t li = min(q0 + u, n_q - 1);
    const int64_t r = qlist ? (int64_t)qlist[li] : li;
    qrow[u] = r;
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      const float4 v = *reinterpret_cast<const float4 *>(F0 + r * C + c);
      q[u][c] = v.x; q[u][c + 1] = v.y; q[u][c + 2] = v.z; q[u][c + 3] = v.w;
    }
  }
  float bd[QPT];
  int bi[QPT];
#pragma unroll
  for (int u = 0; u < QPT; ++u) { bd[u] = __builtin_inff(); bi[u] = 0x7fffffff; }

  for (int64_t j0 = j_begin; j0 < j_end; j0 += KNN_TB) {
    const int nrows = (int)min((int64_t)KNN_TB, j_end - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < KNN_TB * C / 4; e += KNN_THREADS) {
      const int row = e / (C / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < nrows) v = *reinterpret_cast<const float4 *>(F1 + (j0 + row) * C + (e % (C / 4)) * 4);
      *reinterpret_cast<float4 *>(tile + e * 4) = v;
    }
    __syncthreads();
    for (int jj = 0; jj < nrows; ++jj) {
      // knn_d2 (knn_common.h) written out so that one LDS read of b serves the QPT queries: this loop is the definition
      // of the result bits, and knn_d2 must keep its operation order
      float d0[QPT], d1[QPT];
#pragma unroll
      for (int u = 0; u < QPT; ++u) { d0[u] = 0.f; d1[u] = 0.f; }
#pragma unroll
      for (int c = 0; c < C; c += 4) {
        const float4 b = *reinterpret_cast<const float4 *>(tile + jj * C + c);  // LDS broadcast
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
          const float e0 = q[u][c] - b.x, e1 = q[u][c + 1] - b.y;
          const float e2 = q[u][c + 2] - b.z, e3 = q[u][c + 3] - b.w;
          d0[u] = fmaf(e0, e0, d0[u]);
          d1[u] = fmaf(e1, e1, d1[u]);
          d0[u] = fmaf(e2, e2, d0[u]);
          d1[u] = fmaf(e3, e3, d1[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < QPT; ++u) {
        const float d = d0[u] + d1[u];
        if (d < bd[u]) { bd[u] = d; bi[u] = (int)(j0 + jj); }  // strict <: first minimal index wins
      }
    }
  }
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    if (q0 + u < n_q && bi[u] != 0x7fffffff)   // the index as a row of the concatenated F1
      atomicMin(best + qrow[u], knn_key(bd[u], bi[u] + (int)d.r0));
  }
}

__global__ void knn1_finish(const u64 *__restrict__ best, KnnBatch B, int squared,
                            int64_t *__restrict__ idx_out, float *__restrict__ dist_out) {
  const KnnPair d = B.p[blockIdx.y];
  const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= d.n0) return;
  const int64_t i = d.q0 + li;
  const u64 k = best[i];
  idx_out[i] = (k == KNN_KEY_NONE) ? d.r0 : (int64_t)(k & 0xffffffffull);  // all-NaN row: the pair's reference 0
  if (dist_out) {
    const float d2 = __uint_as_float((unsigned int)(k >> 32));
    dist_out[i] = squared ? d2 : sqrtf(d2 + 1e-7f);  // pdist 'L2', core/metrics.py:64-65
  }
}

template <int C>
static int knn_launch(dgr_ctx *ctx, const float *F0, const float *F1, const KnnBatch &B, u64 *best,
                      const int32_t *run_flag, hipStream_t stream, const int32_t *qlist = nullptr,
                      const int32_t *qcount = nullptr, int64_t q_begin = 0) {
  constexpr int QPT = (C <= 32) ? 4 : 2;
  const dim3 grid = knn_brute_grid(ctx, B, QPT, INT32_MAX);
  knn1_kernel<C, QPT><<<grid, KNN_THREADS, 0, stream>>>(F0, F1, B, (int)grid.y, best, run_flag, qlist, qcount, q_begin);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}


// ------------------------------------------------------------------------------------------
// C = 32: the bf16-MFMA prefilter of knn_prefilter.h + exact re-evaluation.  Same result as the brute-force kernel
// above, bit for bit, at ~1/8 of its time.  What the 1-NN search adds to the shared passes:
//   pass 1   keeps the per-query minimum m~_j of d~' over the sample (KNN_SUB = 2: the minimum over half of the
//            references has expected rank 2 among all of them).
//   pass 2   emits every (i, j) with d~' <= m~_j + tau_j.  m~_j >= the true minimum of d~', and tau_j bounds twice the
//            worst-case difference between d~ and the f32 distance, so the brute-force arg-min -- including its
//            first-index tie-break among equal f32 distances -- is always in the list (the list only grows with the
//            sampling, ~2 entries per query).
//   exact    one thread per query evaluates sum (a - b)^2 of its candidates exactly like knn1_kernel and merges with
//            the same 64-bit atomicMin key.
// A query that collects more than KNN_SLOTS candidates (the sample minimum ranks low, or many near-ties, e.g. repeated
// structure) is redone exactly through a device-side query list (a few: knn_query_scan_kernel; many: knn1_kernel);
// a non-finite / huge feature makes the brute-force kernel, launched behind, redo the pair's whole search.
// ------------------------------------------------------------------------------------------
// one thread per query row q in [q_begin, q_end) walks its candidate slots (two on average); candidates are rows of the
// concatenated F1, cand / cand_cnt hold row q at q - q_begin
__global__ void __launch_bounds__(256)
    knn_exact_kernel(const float *__restrict__ F0, const float *__restrict__ F1, const int32_t *__restrict__ cand,
                     const int32_t *__restrict__ cand_cnt, int64_t q_begin, int64_t q_end, u64 *__restrict__ best) {
  const int64_t q = q_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= q_end) return;
  const int cnt = min(cand_cnt[q - q_begin], KNN_SLOTS);
  if (cnt <= 0) return;
  float a[32];
  knn_load_row<32>(a, F0 + q * 32);
  u64 key = KNN_KEY_NONE;
  for (int slot = 0; slot < cnt; ++slot) {
    const int i = cand[(q - q_begin) * KNN_SLOTS + slot];
    const float d = knn_d2<32>(a, F1 + (int64_t)i * 32);
    if (d < __builtin_inff()) {   // (distance bits, index): the order of the slots does not matter
      const u64 k2 = knn_key(d, i);
      key = k2 < key ? k2 : key;
    }
  }
  if (key != KNN_KEY_NONE) atomicMin(best + q, key);
}

// queries that collected more candidates than slots (many near-ties): listed for the search's exact fallbacks.
// blockIdx.y = pair; the pair's list (row numbers inside the pair) starts at qlist[q0 - q_begin]
__global__ void knn_overflow_list(const int32_t *__restrict__ cand_cnt, KnnBatch B, int slots, int64_t q_begin,
                                  int32_t *__restrict__ qlist, int32_t *qcount) {
  const KnnPair d = B.p[blockIdx.y];
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < d.n0 && cand_cnt[d.q0 - q_begin + q] > slots)
    qlist[d.q0 - q_begin + atomicAdd(qcount + blockIdx.y, 1)] = (int32_t)q;
}
int knn_list_overflows(const KnnBatch &B, const KnnPlan &P, int slots, hipStream_t stream) {
  dim3 grid((unsigned)dgr_ceil_div(P.n0_max, 256), B.np);
  knn_overflow_list<<<grid, 256, 0, stream>>>(P.cand_cnt, B, slots, P.q_begin, P.qlist, P.qcount);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// ... SHORT lists (<= KNN_SCAN_MAX queries of a pair) by parallelism over the references: workgroup (x, pair) owns
// the x-th of KNN_SCAN_SPLITS slices of the pair's references and, for every listed query in turn, evaluates its slice
// one reference per thread (knn_d2 per distance), reduces the (distance bits, index) keys over
// the workgroup and issues ONE atomicMin.  (The brute-force kernel keeps 4 queries per THREAD: a handful of listed
// queries would cost it one thread's walk over a whole reference split, ~0.1-0.2 ms.)  Longer lists -- many near-ties,
// e.g. repeated structure -- go to the brute-force kernel, which amortises its tiles over 1024 queries per workgroup.
constexpr int KNN_SCAN_MAX = 64, KNN_SCAN_SPLITS = 16;
__global__ void __launch_bounds__(256)
    knn_query_scan_kernel(const float *__restrict__ F0, const float *__restrict__ F1, KnnBatch B, int64_t q_begin,
                          const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount,
                          u64 *__restrict__ best) {
  __shared__ u64 wkey[4];
  const KnnPair d = B.p[blockIdx.y];
  const int n_q = qcount[blockIdx.y];
  if (n_q <= 0 || n_q > KNN_SCAN_MAX) return;
  const int per = (d.n1 + KNN_SCAN_SPLITS - 1) / KNN_SCAN_SPLITS;
  const int j_begin = blockIdx.x * per, j_end = min(d.n1, j_begin + per);
  for (int li = 0; li < n_q; ++li) {
    const int64_t q = d.q0 + qlist[d.q0 - q_begin + li];
    float a[32];
    knn_load_row<32>(a, F0 + q * 32);
    u64 key = KNN_KEY_NONE;
    for (int j = j_begin + (int)threadIdx.x; j < j_end; j += 256) {
      const float dd = knn_d2<32>(a, F1 + (d.r0 + j) * 32);
      if (dd < __builtin_inff()) {
        const u64 k2 = knn_key(dd, j + (int)d.r0);
        key = k2 < key ? k2 : key;   // (distance bits, index): equal distances -> the smallest index
      }
    }
#pragma unroll
    for (int s2 = 32; s2 > 0; s2 >>= 1) {
      const u64 o = __shfl_xor(key, s2, 64);
      key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) wkey[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 k3 = wkey[0];
      for (int w = 1; w < 4; ++w) k3 = wkey[w] < k3 ? wkey[w] : k3;
      if (k3 != KNN_KEY_NONE) atomicMin(best + q, k3);
    }
    __syncthreads();
  }
}

// brute-force kernel behind the LONG lists: its run flag per pair
__global__ void knn_long_list_flags(const int32_t *__restrict__ qcount, int np, int32_t *__restrict__ flags) {
  if ((int)threadIdx.x < np) flags[threadIdx.x] = qcount[threadIdx.x] > KNN_SCAN_MAX;
}

// the pairs of B (all with at least KNN_MIN_REFS references); best is initialised by the caller
static int knn_prefiltered(dgr_ctx *ctx, const float *F0, const float *F1, KnnBatch B, u64 *best, hipStream_t stream) {
  KnnPlan P;
  DGR_CHECK(knn_prefilter_setup<false>(ctx, F0, F1, B, KNN_SLOTS, stream, &P));
  DGR_CHECK((knn_mfma_launch<false, false>(ctx, B, P, KNN_SUB, KNN_SLOTS, stream)));
  DGR_CHECK((knn_mfma_launch<true, false>(ctx, B, P, 1, KNN_SLOTS, stream)));
  knn_exact_kernel<<<(int)dgr_ceil_div(P.span, 256), 256, 0, stream>>>(F0, F1, P.cand, P.cand_cnt, P.q_begin,
                                                                      P.q_begin + P.span, best);
  DGR_LAUNCH_CHECK();
  // queries with more candidates than slots are redone exactly: short lists (the normal case: empty) by
  // knn_query_scan_kernel, long ones by the brute-force kernel behind its run flag
  DGR_CHECK(knn_list_overflows(B, P, KNN_SLOTS, stream));
  dim3 grid(KNN_SCAN_SPLITS, B.np);
  knn_query_scan_kernel<<<grid, 256, 0, stream>>>(F0, F1, B, P.q_begin, P.qlist, P.qcount, best);
  knn_long_list_flags<<<1, 64, 0, stream>>>(P.qcount, B.np, P.flags);
  DGR_LAUNCH_CHECK();
  DGR_CHECK(knn_launch<32>(ctx, F0, F1, B, best, P.flags, stream, P.qlist, P.qcount, P.q_begin));
  // non-finite / huge input: the brute-force kernel redoes the pair's whole search
  DGR_CHECK(knn_launch<32>(ctx, F0, F1, B, best, P.fallback, stream));
  return knn_trace_prefiltered(ctx, B, P, stream);
}

// Batched entry of the fused pipeline: pair p = rows off0[p] .. off0[p + 1] of F0 against rows off1[p] .. off1[p + 1] of
// F1; idx_out [off0[npairs]] = rows of F1 in the concatenated numbering (what the 6-D assembly gathers with)
int dgr_knn1_batch_impl(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1, const int64_t *off1,
                        int npairs, int C, int squared, int64_t *idx_out, float *dist_out, hipStream_t stream) {
  return knn_for_each_table(ctx, off0, off1, npairs, 1, true, stream, [&](const KnnBatch &B, u64 *best) -> int {
    DGR_CHECK(knn_dispatch(
        B, C,
        [&](auto width, const KnnBatch &pairs) {
          return knn_launch<decltype(width)::value>(ctx, F0, F1, pairs, best, nullptr, stream);
        },
        [&](const KnnBatch &pairs) { return knn_prefiltered(ctx, F0, F1, pairs, best, stream); }));
    dim3 grid((unsigned)dgr_ceil_div(knn_n0_max(B), 256), B.np);
    knn1_finish<<<grid, 256, 0, stream>>>(best, B, squared, idx_out, dist_out);
    DGR_LAUNCH_CHECK();
    return DGR_OK;
  });
}

int dgr_knn1_impl(dgr_ctx *ctx, const float *F0, int64_t N0, const float *F1, int64_t N1, int C,
                  int squared, int64_t *idx_out, float *dist_out, hipStream_t stream) {
  const int64_t off0[2] = {0, N0}, off1[2] = {0, N1};
  return dgr_knn1_batch_impl(ctx, F0, off0, F1, off1, 1, C, squared, idx_out, dist_out, stream);
}

extern "C" int dgr_knn1_l2(dgr_ctx *ctx, const float *F0, int64_t N0, const float *F1, int64_t N1, int C,
                           int squared, int64_t *idx_out, float *dist_out, dgr_stream stream) {
  const int64_t off0[2] = {0, N0}, off1[2] = {0, N1};
  DGR_CHECK(knn_enter("dgr_knn1_l2", ctx, F0, F1, idx_out, off0, off1, 1));
  return dgr_knn1_impl(ctx, F0, N0, F1, N1, C, squared, idx_out, dist_out, (hipStream_t)stream);
}

extern "C" int dgr_knn1_l2_batch(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1,
                                 const int64_t *off1, int npairs, int C, int squared, int64_t *idx_out,
                                 float *dist_out, dgr_stream stream) {
  DGR_CHECK(knn_enter("dgr_knn1_l2_batch", ctx, F0, F1, idx_out, off0, off1, npairs));
  return dgr_knn1_batch_impl(ctx, F0, off0, F1, off1, npairs, C, squared, idx_out, dist_out, (hipStream_t)stream);
}
