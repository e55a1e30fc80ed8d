// Definitions shared by the feature-space k-NN searches: knn.hip (1-NN) and knn_topk.hip (top-k).
#pragma once
#include "dgr_internal.h"

constexpr int KNN_THREADS = 256;
constexpr int KNN_TB = 64;  // F1 rows per LDS tile
constexpr int KNN_MAXP = 32;   // pairs per launch (descriptor table passed by value: no upload, no host buffer to keep alive)

struct KnnPair {
  int64_t q0, r0;      // first query row (of F0) / first reference row (of F1) of the pair
  int32_t n0, n1;      // queries / references
  int32_t qb0, rt0;    // first 32-row block of the pair in the packed query / reference arrays
};
struct KnnBatch {
  KnnPair p[KNN_MAXP];
  int np;
};

// bf16 split-operand prefilter (see the header comment of knn.hip)
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
constexpr float KNN_TAU_C = 8e-5f;  // 2 c
constexpr int KNN_ST = 4;   // reference tiles per LDS stage of the MFMA passes

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

// knn.hip: packs the queries / references of every pair of B into MFMA operand order (32-row tiles, bf16 hi / lo, norms;
// skew: reference layout, see knn_pack_kernel); rows_max = the largest pair's row count rounded up to 32
int knn_pack(const float *F0, const float *F1, const KnnBatch &B, int rows_max, int skew, bf16x8 *Qp, bf16x8 *Rp,
             float *na, float *nb, uint32_t *nb_max, int32_t *fallback, hipStream_t stream);
