// Kernel-volume-1 convs of ResUNetBN2C for gfx950 (conv1_tr and final, the two convs without a kernel map):
// identity_conv_kernel behind dgr_conv_identity_launch, weights in the rule-major kernel's layout (conv.hip) with K = 1;
// and l2_normalize_kernel (dgr_l2_normalize_rows) for unit-norm features wider than the conv's own epilogue covers.
#include <algorithm>

#include "conv_vec.h"
#include "dgr_internal.h"

// ------------------------------------------------------------------------------------------
// Kernel-volume-1 convs (conv1_tr, final: MinkowskiConvolution with kernel_size 1 = a dense [N, Cin] x [Cin, Cout]
// product over the rows of ONE map, model/resunet.py:565-596): a streaming kernel.  No kernel map, no index ring, no
// LDS: a wave takes 32 consecutive rows, every lane requests its 16-byte pieces of them straight into the B-operand
// registers of v_mfma_f32_32x32x2_f32 (lane = row (lane & 31), input channels 8 j + 4 (lane >> 5) .. + 3 -- the layout
// the rule-major kernel builds in LDS), all CP / 8 requests of a tile in flight at once; the layer's weights stay in
// registers for all the tiles of the wave.  Same operands in the same order as sparse_conv_mfma_v2 on an identity map:
// bit-identical results, HBM-bound instead of latency-bound (195 k rows, 96 -> 64: 51 -> ~25 us).
// ------------------------------------------------------------------------------------------
template <int CP, int NBLK>
__global__ void __launch_bounds__(256) identity_conv_kernel(ConvKArgs a) {
  constexpr int S = CP / 8;
  const int lane = threadIdx.x & 63;
  const int n_rows = *a.n_rows_dev;
  const int n_tiles = (n_rows + 31) >> 5;
  const int wave_id = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (int)((gridDim.x * blockDim.x) >> 6);
  f32x4 w[S][NBLK];
  {
    const f32x4 *wp = reinterpret_cast<const f32x4 *>(a.w) + lane;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int j = 0; j < NBLK; ++j) w[s][j] = wp[(s * NBLK + j) * 64];
  }
  const int relu_lo = a.in_relu ? 0 : (int)0x80000000;   // pending ReLU of the producer as one integer max per value
  auto request = [&](int t, f32x4 (&x)[S]) {
    const int64_t row = min((int64_t)t * 32 + (lane & 31), (int64_t)n_rows - 1);   // rows past the end: the last row again
    const float *src = a.in + row * a.in_ld + 4 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < S; ++s) x[s] = *reinterpret_cast<const f32x4 *>(src + 8 * s);
  };
  f32x4 xa[S], xb[S];
  auto tile = [&](int t, f32x4 (&x)[S]) {
    f32x16 acc[NBLK];
#pragma unroll
    for (int j = 0; j < NBLK; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      i32x4 v = __builtin_bit_cast(i32x4, x[s]);
      v.x = max(v.x, relu_lo); v.y = max(v.y, relu_lo); v.z = max(v.z, relu_lo); v.w = max(v.w, relu_lo);
      const f32x4 xv = __builtin_bit_cast(f32x4, v);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < NBLK; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s][j][c], xv[c], acc[j], 0, 0, 0);
    }
    // D column (row of the tile) = lane & 31, D row (channel) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const int64_t row = (int64_t)t * 32 + (lane & 31);
    if (a.l2_normalize) {
      // the feature row of the `final` conv leaves unit-norm (model/resunet.py:643-647): a row's <= 32 channels sit in
      // lanes l and l ^ 32 -- shift first, one cross-lane add, one division per value
      float ss = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int col = 8 * g + 4 * (lane >> 5) + u;
          float v = acc[0][4 * g + u] + ((a.shift && col < a.cout) ? a.shift[col] : 0.f);
          if (col >= a.cout) v = 0.f;
          acc[0][4 * g + u] = v;
          ss += v * v;
        }
      ss += __shfl_xor(ss, 32, 64);
      const float den = sqrtf(ss) + 1e-8f;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[0][e] = acc[0][e] / den;
    }
    if (row < n_rows) {
      float *dst = a.out + row * a.out_ld;
#pragma unroll
      for (int j = 0; j < NBLK; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = 32 * j + 8 * g + 4 * (lane >> 5);
          f32x4 v = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
          if (col + 3 < a.cout && (a.out_ld & 3) == 0) {
            if (a.shift && !a.l2_normalize) v += *reinterpret_cast<const f32x4 *>(a.shift + col);
            *reinterpret_cast<f32x4 *>(dst + col) = v;
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (col + u < a.cout) dst[col + u] = v[u] + ((a.shift && !a.l2_normalize) ? a.shift[col + u] : 0.f);
          }
        }
    }
  };
  // two tiles in flight: the next tile's rows are requested before this tile is multiplied
  int t = wave_id;
  if (t < n_tiles) request(t, xa);
  for (; t < n_tiles; t += 2 * n_waves) {
    const int t1 = t + n_waves;
    if (t1 < n_tiles) request(t1, xb);
    tile(t, xa);
    if (t1 < n_tiles) {
      if (t1 + n_waves < n_tiles) request(t1 + n_waves, xa);
      tile(t1, xb);
    }
  }
}

template <int CP, int NBLK>
static int launch_identity(const ConvKArgs &ka, int64_t rows_cap, int num_cus, hipStream_t stream) {
  // enough waves to keep every CU's memory pipe full, at least two tiles each where the tensor allows it
  int64_t blocks = std::min<int64_t>((int64_t)num_cus * 4, std::max<int64_t>(1, dgr_ceil_div(rows_cap, 32 * 4 * 2)));
  identity_conv_kernel<CP, NBLK><<<(int)blocks, 256, 0, stream>>>(ka);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// The three shapes ResUNetBN2C has (net.hip: LAYERS): conv1_tr reads CAT1 (96 channels, row stride 96) into 64, final reads
// H (64, stride 64) into the caller's <= 64 output channels.  Anything else is refused.
int dgr_conv_identity_launch(const DgrConvLaunch &a, int num_cus, hipStream_t stream, const char **kernel_name) {
  DGR_REQUIRE(a.pair_in == nullptr && a.n_rows_dev != nullptr && a.tile_bound > 0,
              "identity conv: needs a row count and its bound, and no kernel map");
  DGR_REQUIRE(!a.l2_normalize || (a.cout <= 32 && a.cout_pad == 32), "fused l2 normalisation needs Cout <= 32 (got %d)", a.cout);
  const ConvKArgs ka = dgr_conv_kargs(a);
  if (((a.cin | a.in_ld) & 3) == 0 && a.cin == a.cin_pad) {   // rows are read in 16-byte pieces, all CP channels of them
#define DGR_ID(CPV, NBV)                                                                          \
  if (a.cin_pad == CPV && a.cout_pad == 32 * NBV) {                                               \
    if (kernel_name) *kernel_name = "identity_conv_kernel<" #CPV ", " #NBV ">";                   \
    return launch_identity<CPV, NBV>(ka, a.tile_bound * DGR_TILE_M, num_cus, stream);             \
  }
    DGR_ID(64, 1) DGR_ID(64, 2) DGR_ID(96, 2)
#undef DGR_ID
  }
  dgr_set_error("identity conv: no kernel for Cin %d (row stride %d) -> Cout %d: 64 -> <= 64 and 96 -> 33..64 only, Cin and the "
                "row stride multiples of 4", a.cin, a.in_ld, a.cout);
  return DGR_EINVAL;
}

// F / (||F||_2 + 1e-8) per row, model/resunet.py:643-647.  One row per thread (C <= 64).
__global__ void l2_normalize_kernel(const float *__restrict__ in, int in_ld, float *__restrict__ out,
                                    int out_ld, int c, int relu, const int32_t *n_dev) {
  const int64_t n = *n_dev;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int j = 0; j < c; ++j) {
      float v = in[r * in_ld + j];
      if (relu) v = fmaxf(v, 0.f);
      s += v * v;
    }
    const float den = sqrtf(s) + 1e-8f;
    for (int j = 0; j < c; ++j) {
      float v = in[r * in_ld + j];
      if (relu) v = fmaxf(v, 0.f);
      out[r * out_ld + j] = v / den;
    }
  }
}

int dgr_l2_normalize_rows(const float *in, int in_ld, float *out, int out_ld, int c, int relu,
                          const int32_t *n_dev, int64_t n_cap, hipStream_t stream) {
  int64_t blocks = dgr_ceil_div(n_cap, 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  l2_normalize_kernel<<<(int)blocks, 256, 0, stream>>>(in, in_ld, out, out_ld, c, relu, n_dev);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}
