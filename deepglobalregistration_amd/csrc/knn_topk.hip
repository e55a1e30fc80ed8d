// Feature-space k-nearest-neighbour search, 1 < k <= DGR_KNN_MAX_K, exact L2: core.knn.find_knn_gpu(..., knn=k) of the
// reference (core/knn.py:23-74), which repeats `min` k times over the full [chunk, N1] distance matrix.
//
// Every query keeps a sorted list of K packed keys (D2 bits << 32 | row of the concatenated F1) in registers, K = k
// rounded up to a power of two.  D2 is evaluated in the very operation order of knn1_kernel (knn.hip), so the keys order
// like (f32 D2, index) -- equal distances: the smaller index first, like torch.min on the CPU -- and column 0 is the
// 1-NN result bit for bit.  Only finite distances enter a list (the 1-NN kernels' `d < best` with best = inf).
//
// Brute force (every C): knn_topk_kernel, the tile loop of knn1_kernel with a list instead of a (min, argmin) pair.
// F1 is split over workgroups; a 64-bit atomicMin cannot merge lists, so every split writes its partial lists to
// scratch and knn_topk_merge combines them.
//
// Prefilter (C = 32, N1 >= 1024, the policy of the 1-NN search): the bf16-MFMA passes of knn.hip with a top-k bound.
//   pack     knn_pack_kernel with skew = 1: slot s of reference tile t holds row ((s + t) mod 32) n_tiles + t, so that
//            the 32 SLOT CLASSES (rows sitting in slot s of some tile) are disjoint and each is spread over the cloud.
//   pass 1   over a sample of the tiles (every SUB-th stage), the minimum of d~' per query and slot class: 32 minima,
//            attained by 32 distinct reference rows.  knn_topk_bound takes U = the k-th smallest of them.
//   pass 2   every (i, j) with d~'(i, j) <= U_j + tau_j goes to the query's candidate list (slots: 16 K).
//   exact    one thread per query re-evaluates its candidates exactly and keeps the K smallest keys.
// Why the list holds the exact top k (the 1-NN argument of knn.hip, carried over): k distinct rows r_1 .. r_k have
// d~'(r_m) <= U.  The split error gives |d~'(r) + na_j - D2(r)| <= tau_j / 2 for every row r, so
// D2(r_m) <= U + na_j + tau_j / 2 and the k-th smallest exact D2 satisfies D2_(k) <= U + na_j + tau_j / 2.  Every row of
// the exact top k -- ties at D2_(k) under the index order included -- has D2(r) <= D2_(k), hence
// d~'(r) <= D2(r) - na_j + tau_j / 2 <= U + tau_j, and is emitted by pass 2.  The candidate list is therefore a superset
// of the exact top k and the exact pass returns the brute-force keys bit for bit.
// Fallbacks, no host round trip: a query with more candidates than slots is redone by knn_topk_scan_kernel (one
// workgroup per query, exact); a pair with non-finite / huge input, or with more than KNN_TOPK_SCAN_MAX such queries, is
// redone whole by the brute-force kernel behind (run flag per pair).
#include "knn_common.h"

typedef unsigned long long u64;
constexpr u64 KNN_KEY_NONE = ~0ull;
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

// sum_c (a_c - b_c)^2 in the operation order of knn1_kernel (two interleaved fma chains, then one add)
template <int C>
__device__ __forceinline__ float topk_d2(const float (&a)[C], const float *__restrict__ b) {
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
  for (int u = 0; u < QPT; ++u) {
    const int64_t r = min(ql0 + u, N0 - 1);
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      const float4 v = *reinterpret_cast<const float4 *>(F0p + r * C + c);
      q[u][c] = v.x; q[u][c + 1] = v.y; q[u][c + 2] = v.z; q[u][c + 3] = v.w;
    }
  }
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
      const unsigned int ridx = (unsigned int)(j0 + jj + d.r0);   // row of the concatenated F1
#pragma unroll
      for (int u = 0; u < QPT; ++u) {
        const float dd = topk_d2<C>(q[u], tile + jj * C);   // LDS broadcast
        if (dd < __builtin_inff()) topk_insert<K>(L[u], ((u64)__float_as_uint(dd) << 32) | ridx);
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

// host: span of query rows of B in the concatenated F0
static void knn_topk_span(const KnnBatch &B, int64_t *q_begin, int64_t *q_end) {
  *q_begin = B.p[0].q0;
  *q_end = 0;
  for (int p = 0; p < B.np; ++p) {
    *q_begin = std::min(*q_begin, B.p[p].q0);
    *q_end = std::max(*q_end, B.p[p].q0 + B.p[p].n0);
  }
}

template <int C, int K>
static int knn_topk_brute(dgr_ctx *ctx, const float *F0, const float *F1, const KnnBatch &B, int k, u64 *keys,
                          const int32_t *run_flag, hipStream_t stream) {
  constexpr int QPT = knn_topk_qpt(C, K);
  int64_t n0_max = 0, n1_max = 0, qblocks_all = 0, q_begin, q_end;
  for (int p = 0; p < B.np; ++p) {
    n0_max = std::max<int64_t>(n0_max, B.p[p].n0);
    n1_max = std::max<int64_t>(n1_max, B.p[p].n1);
    qblocks_all += dgr_ceil_div(B.p[p].n0, (int64_t)KNN_THREADS * QPT);
  }
  knn_topk_span(B, &q_begin, &q_end);
  const int64_t span = q_end - q_begin;
  // as knn_launch: enough (query block, split) workgroups to cover every CU a few times over
  int splits = (int)dgr_ceil_div((int64_t)ctx->num_cus * 4, qblocks_all);
  splits = (int)std::min<int64_t>(splits, std::min<int64_t>(KNN_TOPK_MAX_SPLITS, dgr_ceil_div(n1_max, KNN_TB)));
  if (splits < 1) splits = 1;
  u64 *part;
  DGR_ALLOC(part, ctx->arena, u64, (int64_t)splits * span * k);
  dim3 grid((unsigned)dgr_ceil_div(n0_max, (int64_t)KNN_THREADS * QPT), splits, B.np);
  knn_topk_kernel<C, K, QPT><<<grid, KNN_THREADS, 0, stream>>>(F0, F1, B, splits, k, q_begin, span, part, run_flag);
  DGR_LAUNCH_CHECK();
  dim3 mgrid((unsigned)dgr_ceil_div(n0_max, 256), B.np);
  knn_topk_merge<K><<<mgrid, 256, 0, stream>>>(part, B, splits, k, q_begin, span, run_flag, keys);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// ------------------------------------------------------------------------------------------
// prefilter (C = 32).  Per-query scratch is addressed by q - q_begin inside its own allocation.
// ------------------------------------------------------------------------------------------
// Grid as knn_mfma_kernel (knn.hip): x = groups of 16 query blocks, y = reference splits, z = pair.
// Pass 1 (PASS2 = false) walks every sub-th stage of its split and leaves the minimum of d~' per query and slot class in
// mt[s * span + q - q_begin] (order-preserving bits, atomicMin over the splits); pass 2 walks every stage and emits the
// rows with d~' <= thr[q - q_begin] into cand[(q - q_begin) * slots ..].
template <bool PASS2>
__global__ void __launch_bounds__(256, 2)
    knn_topk_mfma_kernel(const bf16x8 *__restrict__ Qp, const bf16x8 *__restrict__ Rp, const float *__restrict__ nbp,
                         KnnBatch B, int splits, int sub, int64_t q_begin, int64_t span, uint32_t *__restrict__ mt,
                         const float *__restrict__ thr_q, int32_t *__restrict__ cand, int32_t *__restrict__ cand_cnt,
                         int slots) {
  __shared__ bf16x8 sA[2][KNN_ST * 4 * 64];
  __shared__ __attribute__((aligned(16))) float sNb[2][KNN_ST * 32];
  const KnnPair d = B.p[blockIdx.z];
  const int n_qblocks = (d.n0 + 31) >> 5, n_rtiles = (d.n1 + 31) >> 5;
  if ((int)blockIdx.x * 16 >= n_qblocks) return;   // a smaller pair than the grid's largest
  const int64_t N0 = d.n0, N1 = d.n1;
  const bf16x8 *Q = Qp + (int64_t)d.qb0 * 256, *R = Rp + (int64_t)d.rt0 * 256;
  const float *nb = nbp + (int64_t)d.rt0 * 32;
  const int64_t qrow0 = d.q0 - q_begin;   // the pair's first query in the per-query scratch
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
  const int qb0 = (blockIdx.x * 4 + wave) * 4;     // may lie beyond n_qblocks: clamped loads, guarded outputs
  bf16x8 bq[4][4];
  float m[4][16], thr[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int qb = min(qb0 + u, n_qblocks - 1);
#pragma unroll
    for (int f = 0; f < 4; ++f) bq[u][f] = Q[((int64_t)qb * 4 + f) * 64 + lane];
#pragma unroll
    for (int e = 0; e < 16; ++e) m[u][e] = __builtin_inff();
    thr[u] = 0.f;
    if (PASS2) {
      const int64_t q = (int64_t)qb * 32 + (lane & 31);
      thr[u] = (q < N0 && qb0 + u < n_qblocks) ? thr_q[qrow0 + q] : -__builtin_inff();
    }
  }
  const int n_stages = (n_rtiles + KNN_ST - 1) / KNN_ST;
  const int sps = (n_stages + splits - 1) / splits;   // stages per split
  const int s_begin = blockIdx.y * sps, s_end = min(n_stages, s_begin + sps);
  const int step = PASS2 ? 1 : sub;
  const int s_first = PASS2 ? s_begin : s_begin + min((int)(blockIdx.y % sub), max(s_end - s_begin - 1, 0));
  if (s_first >= s_end) return;   // block-uniform
  bf16x8 pre[KNN_ST];
  float pre_nb = 0.f;
  auto request = [&](int t0) {
#pragma unroll
    for (int j = 0; j < KNN_ST; ++j) pre[j] = R[(int64_t)min(t0 + j, n_rtiles - 1) * 256 + tid];
    if (tid < KNN_ST * 32) pre_nb = nb[(int64_t)min(t0 + (tid >> 5), n_rtiles - 1) * 32 + (tid & 31)];
  };
  auto deposit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < KNN_ST; ++j) sA[buf][j * 256 + tid] = pre[j];
    if (tid < KNN_ST * 32) sNb[buf][tid] = pre_nb;
  };
  request(s_first * KNN_ST);
  deposit(0);
  __syncthreads();
  int buf = 0;
  for (int st = s_first; st < s_end; st += step) {
    const int t0 = st * KNN_ST;
    if (st + step < s_end) request((st + step) * KNN_ST);
#pragma unroll
    for (int j = 0; j < KNN_ST; ++j) {
      const int t = t0 + j;
      if (t >= n_rtiles) break;   // block-uniform
      const bf16x8 a0 = sA[buf][(j * 4 + 0) * 64 + lane], a1 = sA[buf][(j * 4 + 1) * 64 + lane];
      const bf16x8 a2 = sA[buf][(j * 4 + 2) * 64 + lane], a3 = sA[buf][(j * 4 + 3) * 64 + lane];
      f32x16_t c0;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4 *>(&sNb[buf][j * 32 + 8 * g + 4 * h]);
        c0[4 * g] = v.x; c0[4 * g + 1] = v.y; c0[4 * g + 2] = v.z; c0[4 * g + 3] = v.w;
      }
      // the products of knn_mfma_kernel, in its order: identical bits
      f32x16_t acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bq[u][0], c0, 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bq[u][1], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bq[u][2], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bq[u][3], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, bq[u][0], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, bq[u][1], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!PASS2) {
          // element e of lane (query, h) is slot s = (e & 3) + 8 (e >> 2) + 4 h of tile t: one class per element
#pragma unroll
          for (int e = 0; e < 16; ++e) m[u][e] = fminf(m[u][e], acc[u][e]);
        } else {
          float bm = fminf(fminf(acc[u][0], acc[u][1]), fminf(acc[u][2], acc[u][3]));
#pragma unroll
          for (int e = 4; e < 16; e += 4)
            bm = fminf(bm, fminf(fminf(acc[u][e], acc[u][e + 1]), fminf(acc[u][e + 2], acc[u][e + 3])));
          if (!(bm > thr[u])) {
            const int64_t q = (int64_t)(qb0 + u) * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int s = (e & 3) + 8 * (e >> 2) + 4 * h;
              const int64_t i = (int64_t)((s + t) & 31) * n_rtiles + t;   // the skewed layout of knn_pack_kernel
              if (!(acc[u][e] > thr[u]) && q < N0 && i < N1 && qb0 + u < n_qblocks) {
                const int slot = atomicAdd(cand_cnt + qrow0 + q, 1);
                if (slot < slots) cand[(qrow0 + q) * slots + slot] = (int32_t)(i + d.r0);   // beyond: overflow list
              }
            }
          }
        }
      }
    }
    if (st + step < s_end) deposit(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  if (!PASS2) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = (int64_t)(qb0 + u) * 32 + (lane & 31);
      if (qb0 + u < n_qblocks && q < N0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int s = (e & 3) + 8 * (e >> 2) + 4 * h;
          atomicMin(mt + (int64_t)s * span + qrow0 + q, knn_ord(m[u][e]));   // consecutive queries: coalesced
        }
      }
    }
  }
}

// one thread per query: U = the k-th smallest of the 32 class minima, thr = U + tau (tau as in knn_mfma_kernel)
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
#pragma unroll
  for (int c = 0; c < 32; c += 4) {
    const float4 v = *reinterpret_cast<const float4 *>(F0 + q * 32 + c);
    a[c] = v.x; a[c + 1] = v.y; a[c + 2] = v.z; a[c + 3] = v.w;
  }
  u64 L[K];
#pragma unroll
  for (int m = 0; m < K; ++m) L[m] = KNN_KEY_NONE;
  const int32_t *cq = cand + (q - q_begin) * slots;
  for (int s = 0; s < cnt; ++s) {
    const int i = cq[s];
    const float dd = topk_d2<32>(a, F1 + (int64_t)i * 32);
    if (dd < __builtin_inff()) topk_insert<K>(L, ((u64)__float_as_uint(dd) << 32) | (unsigned int)i);
  }
#pragma unroll
  for (int m = 0; m < K; ++m)
    if (m < k) keys[q * k + m] = L[m];
}

// queries with more candidates than slots: qlist[q0 - q_begin + n] = their pair-local rows, qcount[pair] = n
__global__ void knn_topk_overflow_list(const int32_t *__restrict__ cand_cnt, KnnBatch B, int slots, int64_t q_begin,
                                       int32_t *__restrict__ qlist, int32_t *qcount) {
  const KnnPair d = B.p[blockIdx.y];
  const int64_t ql = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ql < d.n0 && cand_cnt[d.q0 - q_begin + ql] > slots)
    qlist[d.q0 - q_begin + atomicAdd(qcount + blockIdx.y, 1)] = (int32_t)ql;
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
#pragma unroll
  for (int c = 0; c < 32; c += 4) {
    const float4 v = *reinterpret_cast<const float4 *>(F0 + q * 32 + c);
    a[c] = v.x; a[c + 1] = v.y; a[c + 2] = v.z; a[c + 3] = v.w;
  }
  u64 L[K];
#pragma unroll
  for (int m = 0; m < K; ++m) L[m] = KNN_KEY_NONE;
  for (int j = (int)threadIdx.x; j < d.n1; j += 256) {
    const float dd = topk_d2<32>(a, F1 + (d.r0 + j) * 32);
    if (dd < __builtin_inff()) topk_insert<K>(L, ((u64)__float_as_uint(dd) << 32) | (unsigned int)(j + d.r0));
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
  DgrArena &arena = ctx->arena;
  int64_t q_begin, q_end;
  knn_topk_span(B, &q_begin, &q_end);
  int n_qb = 0, n_rt = 0, qb_max = 0, rt_max = 0;
  int64_t n0_max = 0;
  for (int p = 0; p < B.np; ++p) {
    KnnPair &d = B.p[p];
    d.qb0 = n_qb;
    d.rt0 = n_rt;
    const int qb = (d.n0 + 31) / 32, rt = (d.n1 + 31) / 32;
    n_qb += qb;
    n_rt += rt;
    qb_max = std::max(qb_max, qb);
    rt_max = std::max(rt_max, rt);
    n0_max = std::max<int64_t>(n0_max, d.n0);
  }
  // per-query arrays span the query rows of B (rows of small pairs in between included: their counts stay zero)
  const int64_t span = q_end - q_begin;
  bf16x8 *Qp, *Rp;
  float *na, *nb, *thr;
  uint32_t *mt;
  int32_t *cand, *cand_cnt, *qlist, *flags;
  DGR_ALLOC(Qp, arena, bf16x8, (int64_t)n_qb * 256);
  DGR_ALLOC(Rp, arena, bf16x8, (int64_t)n_rt * 256);
  DGR_ALLOC(na, arena, float, (int64_t)n_qb * 32);
  DGR_ALLOC(nb, arena, float, (int64_t)n_rt * 32);
  DGR_ALLOC(mt, arena, uint32_t, 32 * span);
  DGR_ALLOC(thr, arena, float, span);
  DGR_ALLOC(qlist, arena, int32_t, span);
  DGR_ALLOC(cand_cnt, arena, int32_t, span + 4 * KNN_MAXP);   // + per pair: max nb bits, fallback flag, overflow count, redo flag
  DGR_ALLOC(cand, arena, int32_t, span * SLOTS);
  uint32_t *nb_max = reinterpret_cast<uint32_t *>(cand_cnt + span);
  int32_t *fallback = cand_cnt + span + KNN_MAXP, *qcount = cand_cnt + span + 2 * KNN_MAXP;
  flags = cand_cnt + span + 3 * KNN_MAXP;
  DGR_HIP_CHECK(hipMemsetAsync(cand_cnt, 0, (size_t)(span + 4 * KNN_MAXP) * sizeof(int32_t), stream));
  DGR_HIP_CHECK(hipMemsetAsync(mt, 0xff, (size_t)(32 * span) * sizeof(uint32_t), stream));
  DGR_CHECK(knn_pack(F0, F1, B, std::max(qb_max, rt_max) * 32, 1, Qp, Rp, na, nb, nb_max, fallback, stream));

  int qgroups_all = 0;
  for (int p = 0; p < B.np; ++p) qgroups_all += (int)dgr_ceil_div((B.p[p].n0 + 31) / 32, 16);
  const int qgroups = (int)dgr_ceil_div(qb_max, 16);
  // reference splits as knn_prefiltered: the count (<= 16) whose grid fills whole rounds of resident workgroups best
  auto launch = [&](auto kernel, int sub) -> int {
    static int per_cu = 0;
    if (per_cu == 0) {
      int n = 0;
      DGR_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0));
      per_cu = n < 1 ? 1 : n;
    }
    const int capacity = ctx->num_cus * per_cu;
    const int stages = (int)dgr_ceil_div(rt_max, KNN_ST);
    int splits = 1;
    double best_fill = 0.;
    for (int sp = 1; sp <= std::min(16, std::max(1, stages / sub)); ++sp) {
      const int64_t blocks = (int64_t)qgroups_all * sp;
      const double fill = (double)blocks / (double)(dgr_ceil_div(blocks, (int64_t)capacity) * capacity);
      if (fill >= best_fill) { best_fill = fill; splits = sp; }
    }
    dim3 grid(qgroups, splits, B.np);
    kernel<<<grid, 256, 0, stream>>>(Qp, Rp, nb, B, splits, sub, q_begin, span, mt, thr, cand, cand_cnt, SLOTS);
    DGR_LAUNCH_CHECK();
    return DGR_OK;
  };
  DGR_CHECK(launch(knn_topk_mfma_kernel<false>, SUB));
  {
    dim3 grid((unsigned)dgr_ceil_div(n0_max, 256), B.np);
    knn_topk_bound<<<grid, 256, 0, stream>>>(mt, na, nb_max, B, k, q_begin, span, thr);
    DGR_LAUNCH_CHECK();
  }
  DGR_CHECK(launch(knn_topk_mfma_kernel<true>, 1));
  knn_topk_exact_kernel<K><<<(unsigned)dgr_ceil_div(span, 256), 256, 0, stream>>>(F0, F1, cand, cand_cnt, SLOTS, k,
                                                                                 q_begin, q_end, keys);
  DGR_LAUNCH_CHECK();
  {
    dim3 grid((unsigned)dgr_ceil_div(n0_max, 256), B.np);
    knn_topk_overflow_list<<<grid, 256, 0, stream>>>(cand_cnt, B, SLOTS, q_begin, qlist, qcount);
    DGR_LAUNCH_CHECK();
  }
  {
    dim3 grid(KNN_TOPK_SCAN_MAX, B.np);   // normally (almost) empty: the workgroups beyond the list return at once
    knn_topk_scan_kernel<K><<<grid, 256, 0, stream>>>(F0, F1, B, k, q_begin, qlist, qcount, keys);
    knn_topk_redo_flags<<<1, 64, 0, stream>>>(fallback, qcount, B.np, flags);
    DGR_LAUNCH_CHECK();
  }
  return knn_topk_brute<32, K>(ctx, F0, F1, B, k, keys, flags, stream);
}

template <int K>
static int knn_topk_batch(dgr_ctx *ctx, const float *F0, const float *F1, const KnnBatch &B, int C, int k,
                          u64 *keys, hipStream_t stream) {
  switch (C) {
    case 16: return knn_topk_brute<16, K>(ctx, F0, F1, B, k, keys, nullptr, stream);
    case 32: {
      static const bool brute = getenv("DGR_KNN_BRUTE") != nullptr;
      // small reference sets: the brute-force kernel alone (the policy of the 1-NN search)
      KnnBatch big, small;
      big.np = small.np = 0;
      for (int p = 0; p < B.np; ++p) {
        if (brute || B.p[p].n1 < 1024) small.p[small.np++] = B.p[p];
        else big.p[big.np++] = B.p[p];
      }
      if (small.np) DGR_CHECK((knn_topk_brute<32, K>(ctx, F0, F1, small, k, keys, nullptr, stream)));
      if (big.np) DGR_CHECK(knn_topk_prefiltered<K>(ctx, F0, F1, big, k, keys, stream));
      return DGR_OK;
    }
    case 64: return knn_topk_brute<64, K>(ctx, F0, F1, B, k, keys, nullptr, stream);
    default:
      dgr_set_error("find_knn: feature width %d not supported (16, 32, 64)", C);
      return DGR_EINVAL;
  }
}

// pairs = row ranges off0 / off1 (host, starting at 0, none empty) of the concatenated F0 / F1; k in [2, DGR_KNN_MAX_K]
static int knn_topk_impl(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1, const int64_t *off1,
                         int npairs, int C, int k, int squared, int64_t *idx_out, float *dist_out, hipStream_t stream) {
  const int64_t n0 = off0[npairs];
  DGR_REQUIRE(off0[0] == 0 && off1[0] == 0, "find_knn: the row offsets start at 0");
  DGR_REQUIRE(off1[npairs] < (1ll << 31) && n0 < (1ll << 31), "find_knn: N0 / N1 too large");
  u64 *keys;
  DGR_ALLOC(keys, ctx->arena, u64, n0 * k);
  const int K = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32;
  for (int p0 = 0; p0 < npairs; p0 += KNN_MAXP) {
    KnnBatch B;
    B.np = std::min(KNN_MAXP, npairs - p0);
    int64_t n0_max = 0;
    for (int p = 0; p < B.np; ++p) {
      KnnPair &d = B.p[p];
      d.q0 = off0[p0 + p]; d.r0 = off1[p0 + p];
      d.n0 = (int32_t)(off0[p0 + p + 1] - off0[p0 + p]); d.n1 = (int32_t)(off1[p0 + p + 1] - off1[p0 + p]);
      d.qb0 = d.rt0 = 0;
      DGR_REQUIRE(d.n0 > 0 && d.n1 > 0, "find_knn: empty feature matrix (N0=%d, N1=%d)", d.n0, d.n1);
      n0_max = std::max<int64_t>(n0_max, d.n0);
    }
    const DgrArena::Mark mk = ctx->arena.mark();
    switch (K) {
      case 2: DGR_CHECK(knn_topk_batch<2>(ctx, F0, F1, B, C, k, keys, stream)); break;
      case 4: DGR_CHECK(knn_topk_batch<4>(ctx, F0, F1, B, C, k, keys, stream)); break;
      case 8: DGR_CHECK(knn_topk_batch<8>(ctx, F0, F1, B, C, k, keys, stream)); break;
      case 16: DGR_CHECK(knn_topk_batch<16>(ctx, F0, F1, B, C, k, keys, stream)); break;
      default: DGR_CHECK(knn_topk_batch<32>(ctx, F0, F1, B, C, k, keys, stream)); break;
    }
    dim3 grid((unsigned)dgr_ceil_div(n0_max * k, 256), B.np);
    knn_topk_finish<<<grid, 256, 0, stream>>>(keys, B, k, squared, idx_out, dist_out);
    DGR_LAUNCH_CHECK();
    ctx->arena.rewind(mk);
  }
  return DGR_OK;
}

extern "C" int dgr_knn_l2(dgr_ctx *ctx, const float *F0, int64_t N0, const float *F1, int64_t N1, int C, int k,
                          int squared, int64_t *idx_out, float *dist_out, dgr_stream stream) {
  DGR_REQUIRE(ctx && F0 && F1 && idx_out, "dgr_knn_l2: NULL argument");
  DGR_REQUIRE(k >= 1 && k <= DGR_KNN_MAX_K, "dgr_knn_l2: k=%d outside [1, %d]", k, DGR_KNN_MAX_K);
  if (k == 1) return dgr_knn1_l2(ctx, F0, N0, F1, N1, C, squared, idx_out, dist_out, stream);
  DGR_REQUIRE(N0 > 0 && N1 > 0, "find_knn: empty feature matrix (N0=%lld, N1=%lld)", (long long)N0, (long long)N1);
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  const int64_t off0[2] = {0, N0}, off1[2] = {0, N1};
  return knn_topk_impl(ctx, F0, off0, F1, off1, 1, C, k, squared, idx_out, dist_out, (hipStream_t)stream);
}

extern "C" int dgr_knn_l2_batch(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1,
                                const int64_t *off1, int npairs, int C, int k, int squared, int64_t *idx_out,
                                float *dist_out, dgr_stream stream) {
  DGR_REQUIRE(ctx && F0 && F1 && off0 && off1 && idx_out, "dgr_knn_l2_batch: NULL argument");
  DGR_REQUIRE(k >= 1 && k <= DGR_KNN_MAX_K, "dgr_knn_l2_batch: k=%d outside [1, %d]", k, DGR_KNN_MAX_K);
  if (k == 1) return dgr_knn1_l2_batch(ctx, F0, off0, F1, off1, npairs, C, squared, idx_out, dist_out, stream);
  DGR_REQUIRE(npairs >= 1, "dgr_knn_l2_batch: npairs=%d", npairs);
  for (int p = 0; p < npairs; ++p)
    DGR_REQUIRE(off0[p + 1] > off0[p] && off1[p + 1] > off1[p], "find_knn: pair %d has an empty feature matrix", p);
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  return knn_topk_impl(ctx, F0, off0, F1, off1, npairs, C, k, squared, idx_out, dist_out, (hipStream_t)stream);
}
