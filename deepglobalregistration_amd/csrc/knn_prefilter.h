// bf16-MFMA prefilter of the feature-space k-NN searches (C = 32): ONE pack kernel, ONE MFMA kernel and one host-side
// plan, instantiated by knn.hip (1-NN, TOPK = false) and knn_topk.hip (top-k, TOPK = true).  A search with the prefilter
// returns what its brute-force kernel returns, bit for bit, at a fraction of its time:
//   pack     every feature row is split x = hi + lo (+ r, |r| <= 2^-18 |x|) into two bf16 rows, stored
//            in MFMA operand order (32-row tiles); reference rows are pre-scaled by -2 (exact) and
//            carry their squared norm nb.
//   pass 1   d~'(i,j) = nb_i - 2 (hi.hi + hi.lo + lo.hi)  on v_mfma_f32_32x32x16_bf16 (6 per 32 x 32
//            block, accumulator initialised with nb through the C operand) over a SAMPLE of the reference tiles (every
//            sub-th stage): an upper bound of what the search is after -- any upper bound will do for the threshold below.
//   pass 2   the same products for ALL tiles -- the same instructions of the same kernel template, hence identical bits
//            where pass 1 ran; every (i, j) with d~' <= bound_j + tau_j goes to the query's candidate list.
//            tau_j = 2 c (na_j + max nb), c = 4e-5, bounds twice the worst-case difference between d~ and the f32 value
//            the brute-force kernels compute (split residual 3 * 2^-18, f32 accumulation of 96 products, f32 norms; see
//            DESIGN.md), so every row the exact search would return is in the list.
//   exact    the search's own kernel re-evaluates the candidates with knn_d2 / knn_key.
// The two searches differ in what pass 1 keeps and where the bound comes from (`if constexpr (TOPK)` below; the argument
// why each bound is one is with the search), in the slot-to-row mapping of the packed references, and in the slot count
// and sampling step, which are compile-time constants for the 1-NN search and arguments for the top-k search.
// A query that collects more candidates than slots is listed (knn_overflow_list) and redone exactly by the search's
// fallback kernels; a non-finite / huge feature raises the pair's fallback flag.  No host round trip either way.
#pragma once
#include "knn_common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
constexpr float KNN_TAU_C = 8e-5f;  // 2 c
constexpr int KNN_ST = 4;   // reference tiles per LDS stage of the MFMA passes
// 1-NN search: candidate slots per query (every 2nd stage sampled: at most 16 seen on the benchmark's features) and the
// sampling step -- pass 1 visits every KNN_SUB-th group of KNN_ST reference tiles (1: all of them).
// Measured per 4-pair batch (BASELINE configs[1], one box): every stage 0.92 ms, every 2nd 0.83, every 4th
// 1.16 -- the second pass slows down with the number of candidates it has to emit (0.52 -> 0.66 ms) and
// 0.5-2 % of the queries overflow their slots, so the sampling stops paying at a half.
constexpr int KNN_SLOTS = 32;
#ifndef DGR_KNN_SUB
#define DGR_KNN_SUB 2
#endif
constexpr int KNN_SUB = DGR_KNN_SUB;

__device__ __forceinline__ unsigned short knn_f2bf(float x) {  // round to nearest even
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float knn_bf2f(unsigned short h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint32_t knn_ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float knn_unord(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
// slot s = (e & 3) + 8 (e >> 2) + 4 h of tile t is element e of the accumulator of lane (query, h)
__device__ __forceinline__ int knn_acc_slot(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// packed[(tile * 4 + f) * 64 + r + 32 g] = 8 bf16: dims 16 (f & 1) + 8 g .. + 7 of row 32 tile + r,
// f >> 1 = 0: hi, 1: lo.  One thread per (row, g, chunk); the (g = 0, chunk = 0) thread also writes the norm.
// blockIdx.y = 2 pair + side (0: queries, 1: references -- pre-scaled by -2, padded with infinite norms, maximum norm
// of the pair left in nb_max[pair]).
// Reference rows are INTERLEAVED over the tiles: slot s of tile t holds row s n_tiles + t, so that every tile -- and
// every subset of tiles, the sample of pass 1 in particular -- is spread evenly over the cloud.  (Consecutive rows are
// neighbouring voxels with similar descriptors: a sample of whole 128-row stages in row order misses whole
// neighbourhoods, and then every member of the true neighbour's cluster lies under the sampled minimum.)
// TOPK rotates the row blocks per tile: slot s of tile t holds row ((s + t) mod 32) n_tiles + t, so that every SLOT
// CLASS (the rows sitting in slot s of some tile), too, is spread over the cloud, and the 32 classes are disjoint.
template <bool TOPK>
__device__ __forceinline__ int64_t knn_slot_row(int s, int t, int n_tiles) {
  return (int64_t)(TOPK ? (s + t) & 31 : s) * n_tiles + t;
}
template <bool TOPK>
__global__ void __launch_bounds__(256)
    knn_pack_kernel(const float *__restrict__ F0, const float *__restrict__ F1, KnnBatch B,
                    bf16x8 *__restrict__ Qp, bf16x8 *__restrict__ Rp, float *__restrict__ na, float *__restrict__ nb,
                    uint32_t *__restrict__ nb_max, int32_t *__restrict__ fallback) {
  const int pair = blockIdx.y >> 1, side = blockIdx.y & 1;
  const KnnPair d = B.p[pair];
  const int64_t N = side ? d.n1 : d.n0;
  const int64_t n_pad = (N + 31) / 32 * 32;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t row = t >> 2;
  if (row >= n_pad) return;
  const float *F = side ? F1 + d.r0 * 32 : F0 + d.q0 * 32;
  const float scale = side ? -2.f : 1.f;
  const int64_t prow = row;                                   // position in the packed array
  if (side) row = knn_slot_row<TOPK>((int)(prow & 31), (int)(prow >> 5), (int)(n_pad >> 5));   // the reference row that sits there
  bf16x8 *packed = side ? Rp + (int64_t)d.rt0 * 256 : Qp + (int64_t)d.qb0 * 256;
  float *norms = side ? nb + (int64_t)d.rt0 * 32 : na + (int64_t)d.qb0 * 32;
  const int g = (int)(t & 1), ch = (int)((t >> 1) & 1);
  bf16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) { hi[e] = 0; lo[e] = 0; }
  if (row < N) {
    const float *src = F + row * 32 + 16 * ch + 8 * g;
    const float4 v0 = *reinterpret_cast<const float4 *>(src), v1 = *reinterpret_cast<const float4 *>(src + 4);
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // non-finite or huge values (squared norms would overflow): leave the pair's search to the exact kernel
      if (!(fabsf(x[e]) < 1e18f)) fallback[pair] = 1;
      const unsigned short h = knn_f2bf(x[e]);
      const unsigned short l = knn_f2bf(x[e] - knn_bf2f(h));
      hi[e] = (short)knn_f2bf(knn_bf2f(h) * scale);  // scale is a power of two: exact
      lo[e] = (short)knn_f2bf(knn_bf2f(l) * scale);
    }
  }
  const int64_t tile = prow >> 5;
  const int r = (int)(prow & 31);
  packed[(tile * 4 + ch) * 64 + r + 32 * g] = hi;
  packed[(tile * 4 + 2 + ch) * 64 + r + 32 * g] = lo;
  // squared norm of the row: the four threads of a row (consecutive lanes) each sum their eight values, fixed order
  float n = 0.f;
  if (row < N) {
    const float *src = F + row * 32 + 16 * ch + 8 * g;
#pragma unroll
    for (int e = 0; e < 8; ++e) n = fmaf(src[e], src[e], n);
  }
  n += __shfl_xor(n, 1, 64);
  n += __shfl_xor(n, 2, 64);
  if (g == 0 && ch == 0) {
    if (row >= N) n = side ? __builtin_inff() : 0.f;   // padding rows: never a minimum / never a query
    else if (side) atomicMax(nb_max + pair, __float_as_uint(n));  // n >= 0: bit patterns order like values
    norms[prow] = n;
  }
}

// The four waves of a workgroup need the same reference tiles: they are staged through LDS, KNN_ST tiles per
// stage (16.5 KB), double buffered -- one global read per workgroup instead of one per wave (the per-wave
// version ran the L1 at ~2/3 of its bandwidth with four identical request streams).
// Grid: x = groups of 16 query blocks (of the largest pair), y = reference splits, z = pair.  PASS2 = false walks
// every sub-th stage of its split only (the sample), PASS2 = true every stage.  Per-query scratch (mt, thr_q, cand,
// cand_cnt) holds row q of the concatenated F0 at element q - q_begin.
//   1-NN   pass 1 leaves the minimum of d~' per query in mt[q - q_begin] (order-preserving bits, atomicMin over the
//          splits); pass 2 takes its bound from there: thr = mt + tau, tau from na and nb_max.
//   top-k  pass 1 leaves the minimum per query and slot class in mt[s * span + q - q_begin]; pass 2 reads thr_q, which
//          knn_topk_bound (knn_topk.hip) computed from them.
// Pass 2 emits the rows within the bound into cand[(q - q_begin) * slots ..], counted in cand_cnt[q - q_begin].
template <bool PASS2, bool TOPK>
__global__ void __launch_bounds__(256, 2)
    knn_mfma_kernel(const bf16x8 *__restrict__ Qp, const bf16x8 *__restrict__ Rp, const float *__restrict__ nbp,
                    KnnBatch B, int splits, int sub_arg, int64_t q_begin, int64_t span, uint32_t *__restrict__ mt,
                    const float *__restrict__ nap, const uint32_t *__restrict__ nb_max,
                    const float *__restrict__ thr_q, int32_t *__restrict__ cand, int32_t *__restrict__ cand_cnt,
                    int slots_arg) {
  __shared__ bf16x8 sA[2][KNN_ST * 4 * 64];
  __shared__ __attribute__((aligned(16))) float sNb[2][KNN_ST * 32];
  const int sub = TOPK ? sub_arg : KNN_SUB, slots = TOPK ? slots_arg : KNN_SLOTS;   // 1-NN: compile-time constants
  constexpr int NM = TOPK ? 16 : 1;   // pass-1 minima per lane and query block: one per slot class / one
  const KnnPair d = B.p[blockIdx.z];
  const int n_qblocks = (d.n0 + 31) >> 5, n_rtiles = (d.n1 + 31) >> 5;
  if ((int)blockIdx.x * 16 >= n_qblocks) return;   // a smaller pair than the grid's largest
  const int64_t N0 = d.n0, N1 = d.n1;
  const bf16x8 *Q = Qp + (int64_t)d.qb0 * 256, *R = Rp + (int64_t)d.rt0 * 256;
  const float *nb = nbp + (int64_t)d.rt0 * 32;
  const int64_t qrow0 = d.q0 - q_begin;   // the pair's first query in the per-query scratch
  mt += qrow0;
  cand += qrow0 * slots;
  cand_cnt += qrow0;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
  const int qb0 = (blockIdx.x * 4 + wave) * 4;     // may lie beyond n_qblocks: clamped loads, guarded outputs
  bf16x8 bq[4][4];
  float m[4][NM], thr[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int qb = min(qb0 + u, n_qblocks - 1);
#pragma unroll
    for (int f = 0; f < 4; ++f) bq[u][f] = Q[((int64_t)qb * 4 + f) * 64 + lane];
#pragma unroll
    for (int e = 0; e < NM; ++e) m[u][e] = __builtin_inff();
    thr[u] = 0.f;
    if constexpr (PASS2) {
      const int64_t q = (int64_t)qb * 32 + (lane & 31);
      const bool live = q < N0 && qb0 + u < n_qblocks;
      if constexpr (TOPK) {
        thr[u] = live ? thr_q[qrow0 + q] : -__builtin_inff();
      } else {
        const float nmax = __uint_as_float(nb_max[blockIdx.z]);
        thr[u] = live ? knn_unord(mt[q]) + KNN_TAU_C * (nap[(int64_t)d.qb0 * 32 + q] + nmax) : -__builtin_inff();
      }
    }
  }
  // stages (KNN_ST tiles) of this split; pass 1 takes every sub-th of them, offset by the split index so that the
  // sample does not alias with the split length
  const int n_stages = (n_rtiles + KNN_ST - 1) / KNN_ST;
  const int sps = (n_stages + splits - 1) / splits;   // stages per split
  const int s_begin = blockIdx.y * sps, s_end = min(n_stages, s_begin + sps);
  const int step = PASS2 ? 1 : sub;
  // (a pair with fewer than sub stages per split still gets one sampled stage per split)
  const int s_first = PASS2 ? s_begin : s_begin + min((int)(blockIdx.y % sub), max(s_end - s_begin - 1, 0));
  if (s_first >= s_end) return;   // block-uniform
  // stage loader: thread tid fetches piece tid + 256 j of tile t0 + j (contiguous 4 KB per tile) and one norm
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
    if (st + step < s_end) request((st + step) * KNN_ST);   // lands behind this stage's MFMAs
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
      // the six MFMAs of a block form a dependent chain: the four blocks are interleaved step by step so that
      // every MFMA has three independent ones between itself and its predecessor
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
        if constexpr (!PASS2 && TOPK) {   // one slot class per accumulator element
#pragma unroll
          for (int e = 0; e < 16; ++e) m[u][e] = fminf(m[u][e], acc[u][e]);
        } else {
          float bm = fminf(fminf(acc[u][0], acc[u][1]), fminf(acc[u][2], acc[u][3]));
#pragma unroll
          for (int e = 4; e < 16; e += 4)
            bm = fminf(bm, fminf(fminf(acc[u][e], acc[u][e + 1]), fminf(acc[u][e + 2], acc[u][e + 3])));
          if constexpr (!PASS2) {
            m[u][0] = fminf(m[u][0], bm);
          } else if (!(bm > thr[u])) {   // some reference of this block is within the query's bound
            const int64_t q = (int64_t)(qb0 + u) * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int64_t i = knn_slot_row<TOPK>(knn_acc_slot(e, h), t, n_rtiles);   // the layout of knn_pack_kernel
              if (!(acc[u][e] > thr[u]) && q < N0 && i < N1 && qb0 + u < n_qblocks) {
                const int slot = atomicAdd(cand_cnt + q, 1);   // per-query counters: no hot address
                if (slot < slots) cand[q * slots + slot] = (int32_t)(i + d.r0);   // beyond: knn_overflow_list
              }
            }
          }
        }
      }
    }
    if (st + step < s_end) deposit(buf ^ 1);
    __syncthreads();   // the other buffer is complete; this one may be overwritten by the next deposit
    buf ^= 1;
  }
  if constexpr (!PASS2) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = (int64_t)(qb0 + u) * 32 + (lane & 31);
      const bool live = qb0 + u < n_qblocks && q < N0;
      if constexpr (TOPK) {
        if (live) {
#pragma unroll
          for (int e = 0; e < 16; ++e)   // consecutive queries: coalesced
            atomicMin(mt + (int64_t)knn_acc_slot(e, h) * span + q, knn_ord(m[u][e]));
        }
      } else {
        const float mm = fminf(m[u][0], __shfl_xor(m[u][0], 32, 64));   // the two halves of the tile's slots
        if (lane < 32 && live) atomicMin(mt + q, knn_ord(mm));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// Layout and scratch of one prefiltered table of pairs.  Per-query arrays span the query rows of the table in the
// concatenated F0 (not the sum of their rows) and hold row q at element q - q_begin.  Pairs too small for the prefilter
// that sit between large ones are covered as well -- their counts stay zero and the per-row kernels return at once for
// them; the span is at most the batch's N0, which the arena is sized for (DGR_ENOMEM otherwise).
struct KnnPlan {
  int64_t q_begin, span, n0_max;
  int qb_max, rt_max;   // 32-row blocks of the largest query / reference set
  int qgroups_all;      // groups of 16 query blocks over all pairs: the MFMA grids' workgroups per reference split
  bf16x8 *Qp, *Rp;      // packed queries / references; pair p starts at block B.p[p].qb0 / rt0
  float *na, *nb;       // their squared norms
  uint32_t *mt;         // pass-1 minima, order-preserving bits: [span] (1-NN) / [32 slot classes][span] (top-k)
  float *thr;           // top-k only: pass-2 bound per query
  int32_t *qlist, *cand_cnt, *cand;   // overflow list [span], candidate count [span] and slots [span][slots]
  // per pair [KNN_MAXP]: bits of max nb, non-finite / huge input, length of the overflow list, the search's redo flag
  uint32_t *nb_max;
  int32_t *fallback, *qcount, *flags;
};

// lays the pairs of B out in the packed arrays (B.p[].qb0 / rt0), takes the scratch from the arena, clears it and packs
template <bool TOPK>
inline int knn_prefilter_setup(dgr_ctx *ctx, const float *F0, const float *F1, KnnBatch &B, int slots,
                               hipStream_t stream, KnnPlan *plan) {
  KnnPlan &P = *plan;
  DgrArena &arena = ctx->arena;
  int n_qb = 0, n_rt = 0;
  P.qb_max = P.rt_max = P.qgroups_all = 0;
  for (int p = 0; p < B.np; ++p) {
    KnnPair &d = B.p[p];
    d.qb0 = n_qb;
    d.rt0 = n_rt;
    const int qb = (d.n0 + 31) / 32, rt = (d.n1 + 31) / 32;
    n_qb += qb;
    n_rt += rt;
    P.qb_max = std::max(P.qb_max, qb);
    P.rt_max = std::max(P.rt_max, rt);
    P.qgroups_all += (int)dgr_ceil_div(qb, 16);
  }
  P.n0_max = knn_n0_max(B);
  P.span = knn_query_span(B, &P.q_begin);
  const int64_t n_mt = (TOPK ? 32 : 1) * P.span;
  DGR_ALLOC(P.Qp, arena, bf16x8, (int64_t)n_qb * 256);
  DGR_ALLOC(P.Rp, arena, bf16x8, (int64_t)n_rt * 256);
  DGR_ALLOC(P.na, arena, float, (int64_t)n_qb * 32);
  DGR_ALLOC(P.nb, arena, float, (int64_t)n_rt * 32);
  DGR_ALLOC(P.mt, arena, uint32_t, n_mt);
  P.thr = nullptr;
  if (TOPK) DGR_ALLOC(P.thr, arena, float, P.span);
  DGR_ALLOC(P.qlist, arena, int32_t, P.span);
  DGR_ALLOC(P.cand_cnt, arena, int32_t, P.span + 4 * KNN_MAXP);   // the per-pair words behind: one memset clears both
  DGR_ALLOC(P.cand, arena, int32_t, P.span * slots);
  int32_t *pair_words = P.cand_cnt + P.span;
  P.nb_max = reinterpret_cast<uint32_t *>(pair_words);
  P.fallback = pair_words + KNN_MAXP;
  P.qcount = pair_words + 2 * KNN_MAXP;
  P.flags = pair_words + 3 * KNN_MAXP;
  DGR_HIP_CHECK(hipMemsetAsync(P.cand_cnt, 0, (size_t)(P.span + 4 * KNN_MAXP) * sizeof(int32_t), stream));
  DGR_HIP_CHECK(hipMemsetAsync(P.mt, 0xff, (size_t)n_mt * sizeof(uint32_t), stream));
  dim3 grid((unsigned)dgr_ceil_div((int64_t)std::max(P.qb_max, P.rt_max) * 32 * 4, 256), 2 * B.np);
  knn_pack_kernel<TOPK><<<grid, 256, 0, stream>>>(F0, F1, B, P.Qp, P.Rp, P.na, P.nb, P.nb_max, P.fallback);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// One pass of the MFMA kernel over the table.  Reference splits are chosen so that the grid fills the chip in whole
// rounds of resident workgroups (one round when possible): a grid of 1.3 x the resident capacity leaves the second
// round two thirds empty.  The resident workgroups per CU are asked once per kernel instantiation.
template <bool PASS2, bool TOPK>
inline int knn_mfma_launch(dgr_ctx *ctx, const KnnBatch &B, const KnnPlan &P, int sub, int slots, hipStream_t stream) {
  const auto kernel = knn_mfma_kernel<PASS2, TOPK>;
  static int per_cu = 0;
  if (per_cu == 0) {
    int n = 0;
    DGR_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0));
    per_cu = n < 1 ? 1 : n;
  }
  const int capacity = ctx->num_cus * per_cu;
  const int stages = (int)dgr_ceil_div(P.rt_max, KNN_ST);
  // the split count (<= 16) whose grid fills whole rounds of resident workgroups best; ties -> more splits
  int splits = 1;
  double best_fill = 0.;
  for (int sp = 1; sp <= std::min(16, std::max(1, stages / sub)); ++sp) {
    const int64_t blocks = (int64_t)P.qgroups_all * sp;
    const double fill = (double)blocks / (double)(dgr_ceil_div(blocks, (int64_t)capacity) * capacity);
    if (fill >= best_fill) { best_fill = fill; splits = sp; }
  }
  dim3 grid((unsigned)dgr_ceil_div(P.qb_max, 16), splits, B.np);
  kernel<<<grid, 256, 0, stream>>>(P.Qp, P.Rp, P.nb, B, splits, sub, P.q_begin, P.span, P.mt, P.na, P.nb_max, P.thr,
                                   P.cand, P.cand_cnt, slots);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// Route trace of a prefiltered table, called by the searches behind their last launch and BEFORE the arena is rewound:
// waits for the stream, copies cand_cnt and the per-pair words behind it to the host and reduces them into the rows
// knn_trace_table opened (the pair words are indexed by the pair's position in B, the prefiltered sub-batch).
inline int knn_trace_prefiltered(dgr_ctx *ctx, const KnnBatch &B, const KnnPlan &P, hipStream_t stream) {
  if (!ctx->knn_trace) return DGR_OK;
  std::vector<int32_t> host((size_t)(P.span + 4 * KNN_MAXP));
  DGR_HIP_CHECK(hipStreamSynchronize(stream));
  DGR_HIP_CHECK(hipMemcpy(host.data(), P.cand_cnt, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  const int32_t *words = host.data() + P.span;
  const size_t n_table = ctx->knn_trace_q0.size();
  int32_t *rows = ctx->knn_trace_rows.data() + (ctx->knn_trace_rows.size() - n_table * DGR_KNN_TRACE_FIELDS);
  for (int p = 0; p < B.np; ++p) {
    const KnnPair &d = B.p[p];
    size_t t = 0;
    while (t < n_table && ctx->knn_trace_q0[t] != d.q0) ++t;
    DGR_REQUIRE(t < n_table, "find_knn: trace row of a prefiltered pair not found");
    int32_t cnt_max = 0, n_zero = 0;
    for (int64_t q = 0; q < d.n0; ++q) {
      const int32_t c = host[(size_t)(d.q0 - P.q_begin + q)];
      cnt_max = std::max(cnt_max, c);
      n_zero += c == 0;
    }
    int32_t *row = rows + t * DGR_KNN_TRACE_FIELDS;
    row[2] = 1;
    row[3] = words[KNN_MAXP + p];
    row[4] = words[2 * KNN_MAXP + p];
    row[5] = words[3 * KNN_MAXP + p];
    row[6] = cnt_max;
    row[7] = n_zero;
  }
  return DGR_OK;
}

// knn.hip: lists the queries with more than `slots` candidates -- P.qlist[q0 - q_begin + n] = their row inside the pair,
// P.qcount[pair] = n -- for the search's fallback kernels
int knn_list_overflows(const KnnBatch &B, const KnnPlan &P, int slots, hipStream_t stream);
