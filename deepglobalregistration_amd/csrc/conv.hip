// Sparse convolution forward for gfx950, the rule-major two-phase path in exact f32:
// gather -> LDS tile -> f32 MFMA -> per-pair product rows, then a deterministic segmented reduction per output row.
// Replaces the ME.MinkowskiConvolution / MinkowskiConvolutionTranspose forward invoked by every
// conv of ResUNetBN2C (model/resunet.py:598-649, model/residual_block.py:15-80).
//
// This file holds sparse_conv_mfma_v2 with its dispatch (dgr_conv_launch) and the reduction pass (reduce_rows_kernel,
// dgr_reduce_rows) that the wide kernels of conv_wide.hip share.  The rule-major kernel runs the layers the split-operand
// kernels do not cover (the table above dgr_conv_launch); kernel-volume-1 convs are in conv_identity.hip, conv1 with <= 8
// input channels in conv1.hip, the wide 6-D layers in conv_wide.hip, the K = 27 layers of the FCGF net in conv_os.hip.
//
// Phase 1 (sparse_conv_mfma_v2): the kernel map lists pairs (in, out) per kernel offset k ("rule").  A
// tile is <= 64 pairs of ONE rule: the 64 gathered input rows [64 x Cin] are staged in LDS once and
// multiplied with the rule's dense [Cin x Cout] slice on the matrix cores
// (v_mfma_f32_32x32x2_f32: exact f32, bitwise an fma chain); the product rows go to Y[pair, Cout]
// with plain coalesced stores (32 consecutive lanes write 128 consecutive bytes).  The grid is
// persistent and XCD-aware: each of the 8 XCDs walks a contiguous range of tiles, i.e. a contiguous
// range of rules, so a rule's weight slice is pulled into ONE L2.
// Phase 2 (reduce_rows): every output row sums its Y rows in ascending-k order (output-major CSR
// from kmap.hip), starting from the folded batch-norm shift (+ residual), and is written once.
// Measured alternative that this replaces: scatter with global_atomic_add_f32 is capped at ~333 G
// lanes/s chip-wide (tools/microbench/atomic_xcd.hip, independent of XCD locality) and serialises
// with the MFMA phase; plain stores + one streaming pass are faster AND bit-reproducible.
//
// Weight layout (prepared once in net.hip): W[k][s][nb][lane][c], s = Cin_pad/8 K-steps,
// nb = Cout_pad/32 column blocks, value = W_folded[k][8 s + 4 (lane>>5) + c][32 nb + (lane&31)],
// so a wave fetches the B operands of 4 MFMAs with one coalesced 16-byte load per lane.
#include <algorithm>

#include "dgr_internal.h"
#include "split.h"

// sparse_conv_mfma_v2 still carries the identity mode it ran conv1_tr and final in before identity_conv_kernel
// (conv_identity.hip) did.  No launch takes it any more (dgr_conv_launch requires a kernel map), but without it the compiler
// schedules the 256 -> 256 instantiation 2.4 % slower (profiles/README.md, conv_split): the body stays as it was measured.
int dgr_resident_blocks(const void *kernel, int threads, size_t lds_bytes, int *blocks, int num_cus) {
  int per_cu = 0, dev = 0;
  DGR_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes));
  if (num_cus <= 0) {
    DGR_HIP_CHECK(hipGetDevice(&dev));
    DGR_HIP_CHECK(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  *blocks = (per_cu < 1 ? 1 : per_cu) * (num_cus < 1 ? 1 : num_cus);
  return DGR_OK;
}

// Product rows are written once and read once.  Measured on the 256-wide layers (3.7 GB of product rows per
// launch): reading them with non-temporal loads in the reduce pass is 19 % faster (no L2 allocation for data
// that is never touched again); non-temporal STORES in the MFMA kernel cost it 10 % (the 16-byte pieces of a
// row no longer merge in L2) and narrow layers, whose product rows fit the L2 / MALL, prefer plain loads.
template <bool STREAM>
__device__ __forceinline__ f32x4 dgr_y_load(const float *p) {
  if (STREAM) return __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
  return *reinterpret_cast<const f32x4 *>(p);
}
// ------------------------------------------------------------------------------------------
// v2: compile-time Cin, software-pipelined in PHASES of <= 128 input channels.
//   * LDS holds two A buffers [64 rows x CK channels]; phase q multiplies out of buffer q&1 while
//     the rows of phase q+1 (requested one phase earlier, held in <= 8 float4 registers per thread)
//     are dropped into the other buffer and the rows of phase q+2 are requested -> ONE barrier per
//     phase, and every gather has a whole MFMA phase to land.
//   * vmcnt retires in order and store acknowledgements are slow, so the first three B-operand
//     loads of a tile are issued before the previous tile's stores; B runs a 4-deep register ring.
//   * MFMA operands are swapped (D = W^T . In^T): a lane owns one pair and 4 x 4 consecutive output
//     channels, so product rows leave as 16-byte stores.
//   * row indices travel through a 4-slot LDS ring, loaded two tiles ahead.
// ------------------------------------------------------------------------------------------
#define DGR_WIDE_CK 128     // phase width (input channels) of the widest configuration
#define DGR_WIDE_WAVES 2    // waves per SIMD the widest configuration is compiled for (64 / 3 measured within +-1 %)
constexpr int conv_phase_width(int cp, int acc_blocks) {
  const int cap = acc_blocks >= 4 ? DGR_WIDE_CK : 128;
  return cp > cap ? cap : cp;
}

template <int CP, int WM, int WN, int MB, int NB, bool VEC>
__global__ void __launch_bounds__(64 * WM * WN, (MB * NB >= 4 ? DGR_WIDE_WAVES : 1)) sparse_conv_mfma_v2(ConvKArgs a) {
  constexpr int THREADS = 64 * WM * WN;
  constexpr int TM = 32 * MB * WM;
  static_assert(TM == DGR_TILE_M, "tile height must match the kernel-map tiling");
  constexpr int NBLK = NB * WN;
  constexpr int CK = conv_phase_width(CP, MB * NB);  // channels per phase
  constexpr int PPT = CP / CK;                // phases per tile
  static_assert(CP % CK == 0, "phase width must divide Cin");
  constexpr int C4K = CK / 4;                 // 16-byte pieces per row per phase
  constexpr int NCH = TM * C4K / THREADS;     // pieces per thread per phase
  static_assert(TM * C4K % THREADS == 0, "gather pieces must divide evenly");
  constexpr int LDA = CK + 4;
  constexpr int SK = CK / 8;                  // K-steps per phase
  constexpr int S = CP / 8;                   // K-steps per tile
  constexpr int RING = 4;
  static_assert(SK == 1 || SK % RING == 0, "phase length must be a multiple of the B ring");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *As = lds;                                                 // [2][TM][LDA]
  int *idxbuf = reinterpret_cast<int *>(lds + 2 * TM * LDA);       // [4][TM]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const bool identity = (a.pair_in == nullptr);
  const int n_rows = identity ? *a.n_rows_dev : 0;
  const int T = identity ? (n_rows + TM - 1) / TM : a.tile_ptr[a.K];
  const int per = (T + 7) >> 3;
  const int xcd = blockIdx.x & 7;
  const int t_end = min(T, (xcd + 1) * per);
  const int nj = gridDim.x >> 3;
  const int t_first = xcd * per + (blockIdx.x >> 3);
  if (t_first >= t_end) return;
  const int n_my = (t_end - t_first + nj - 1) / nj;  // tiles of this block: t_first + i * nj
  const int NQ = n_my * PPT;                         // phases of this block

  auto locate = [&](int i, int &k, int &pstart, int &count) {
    const int tt = t_first + i * nj;
    if (identity) {
      k = 0;
      pstart = tt * TM;
      count = min(TM, n_rows - pstart);
    } else {
      const int4 d = a.tile_desc[tt];  // one scalar 16-byte load (kmap.hip: tile_desc_kernel)
      k = d.x;
      pstart = d.y;
      count = d.z;
    }
  };
  auto load_idx = [&](int i) -> int {  // input row of tile-row `tid` of the block's i-th tile, or -1
    if (i >= n_my || tid >= TM) return -1;
    int k, pstart, count;
    locate(i, k, pstart, count);
    if (tid >= count) return -1;
    return identity ? pstart + tid : a.pair_in[pstart + tid];
  };
  f32x4 G[NCH];
  uint32_t g_ok = 0;  // bit i: piece i of the requested phase is a real (row, channel) piece
  // Requests only: NOTHING here may consume a loaded value (a consumer right behind the load costs an
  // s_waitcnt vmcnt(0) per piece -- the gather then runs serialised, and behind every B operand in
  // flight).  Invalid pieces are loaded from a clamped address and zeroed in land(); the ReLU-on-read
  // is applied in land() too, one phase later, when the data has long arrived.
  auto gather = [&](int q) {  // request the rows of phase q (tile q / PPT, channels (q % PPT) * CK ..)
    const int *idx = idxbuf + ((q / PPT) & 3) * TM;
    const int cbase = (q % PPT) * CK;
    g_ok = 0;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * THREADS;
      const int r = ch / C4K, c = cbase + (ch % C4K) * 4;
      int row = idx[r];
      if (VEC) {
        const int rr = max(row, 0);
        const int cc = min(c, a.cin - 4);
        G[i] = *reinterpret_cast<const f32x4 *>(a.in + (int64_t)rr * a.in_ld + cc);
        g_ok |= (row >= 0 && c < a.cin) ? (1u << i) : 0u;
      } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row >= 0) {
          const float *src = a.in + (int64_t)row * a.in_ld + c;
          if (c + 0 < a.cin) v.x = src[0];
          if (c + 1 < a.cin) v.y = src[1];
          if (c + 2 < a.cin) v.z = src[2];
          if (c + 3 < a.cin) v.w = src[3];
        }
        G[i] = v;
        g_ok |= 1u << i;
      }
    }
  };
  auto land = [&](int q) {  // registers -> A buffer q & 1
    float *dst = As + (q & 1) * TM * LDA;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * THREADS;
      f32x4 v = G[i];
      if (a.in_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      const bool ok = (g_ok >> i) & 1u;
      v.x = ok ? v.x : 0.f;
      v.y = ok ? v.y : 0.f;
      v.z = ok ? v.z : 0.f;
      v.w = ok ? v.w : 0.f;
      *reinterpret_cast<f32x4 *>(dst + (ch / C4K) * LDA + (ch % C4K) * 4) = v;
    }
  };

  // ---- prologue: indices of tiles 0..2 into the LDS ring, tile 3's into a register; phase 0 landed,
  //      phase 1 in flight; first B operands of tile 0 requested
  {
    const int i0 = load_idx(0), i1 = load_idx(1), i2 = load_idx(2);
    if (tid < TM) { idxbuf[tid] = i0; idxbuf[TM + tid] = i1; idxbuf[2 * TM + tid] = i2; }
  }
  int next_pub = 3;
  int idx_reg = load_idx(3);
  int k, pstart, count;
  locate(0, k, pstart, count);
  f32x4 b[RING][NB];
  {
    const f32x4 *w0 = reinterpret_cast<const f32x4 *>(a.w) + ((int64_t)k * S * NBLK + wn * NB) * 64 + lane;
#pragma unroll
    for (int r = 0; r < RING - 1; ++r)
      if (r < S) {
#pragma unroll
        for (int j = 0; j < NB; ++j) b[r][j] = w0[((int64_t)r * NBLK + j) * 64];
      }
  }
  __syncthreads();
  gather(0);
  land(0);
  if (1 < NQ) gather(1);
  __syncthreads();

  f32x16 acc[MB][NB];
  for (int q = 0; q < NQ; ++q) {
    const int h = q % PPT;
    if (q + 1 < NQ) land(q + 1);      // requested one phase ago
    if (q + 2 < NQ) gather(q + 2);    // a whole phase to arrive
    if ((q + 3) / PPT >= next_pub && next_pub < n_my) {  // indices for the gather of the phase after next
      if (tid < TM) idxbuf[(next_pub & 3) * TM + tid] = idx_reg;
      ++next_pub;
      idx_reg = load_idx(next_pub);
    }
    if (h == 0) {
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    }
    // ---- MFMA over this phase's channels
    const f32x4 *wk = reinterpret_cast<const f32x4 *>(a.w) + ((int64_t)k * S * NBLK + wn * NB) * 64 + lane;
    const float *arow = As + (q & 1) * TM * LDA + (32 * wm * MB + (lane & 31)) * LDA + 4 * (lane >> 5);
    const int s0 = h * SK;
#pragma unroll
    for (int s = 0; s < SK; ++s) {
      if (s0 + s + RING - 1 < S) {
#pragma unroll
        for (int j = 0; j < NB; ++j) b[(s + RING - 1) % RING][j] = wk[((int64_t)(s0 + s + RING - 1) * NBLK + j) * 64];
      }
      // pin the prefetch HERE: without it the scheduler sinks each load next to its first use
      // (load-to-use distance 0, full L2 latency exposed on every K-step; seen in the ISA)
      __builtin_amdgcn_sched_barrier(0);
      f32x4 av[MB];
#pragma unroll
      for (int i = 0; i < MB; ++i) av[i] = *reinterpret_cast<const f32x4 *>(arow + i * 32 * LDA + s * 8);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s % RING][j][c], av[i][c], acc[i][j], 0, 0, 0);
    }
    if (h == PPT - 1) {
      // ---- tile finished: request the next tile's first B operands BEFORE this tile's stores
      const int pst = pstart, cnt = count;
      const int i_next = q / PPT + 1;
      if (i_next < n_my) {
        locate(i_next, k, pstart, count);
        const f32x4 *w1 = reinterpret_cast<const f32x4 *>(a.w) + ((int64_t)k * S * NBLK + wn * NB) * 64 + lane;
#pragma unroll
        for (int r = 0; r < RING - 1; ++r)
          if (r < S) {
#pragma unroll
            for (int j = 0; j < NB; ++j) b[r][j] = w1[((int64_t)r * NBLK + j) * 64];
          }
      }
      // product rows: D column (pair) = lane & 31, D row (channel) = (e&3) + 8 (e>>2) + 4 (lane>>5)
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int r = 32 * (wm * MB + i) + (lane & 31);
        if (identity && a.l2_normalize) {
          // the feature row of the `final` conv leaves unit-norm (model/resunet.py:643-647): a row's <= 32 channels sit
          // in lanes l and l ^ 32 of the one wave column -- shift first, one cross-lane add, one division per value
          float ss = 0.f;
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int col = 8 * g + 4 * (lane >> 5) + u;
              float v = acc[i][0][4 * g + u] + ((a.shift && col < a.cout) ? a.shift[col] : 0.f);
              if (col >= a.cout) v = 0.f;
              acc[i][0][4 * g + u] = v;
              ss += v * v;
            }
          ss += __shfl_xor(ss, 32, 64);
          const float den = sqrtf(ss) + 1e-8f;
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][0][e] = acc[i][0][e] / den;
        }
        if (r < cnt) {
          float *dst = identity ? a.out + (int64_t)(pst + r) * a.out_ld : a.y + (int64_t)(pst + r) * a.y_ld;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int col = 32 * (wn * NB + j) + 8 * g + 4 * (lane >> 5);
              f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
              if (identity) {
                if (col + 3 < a.cout && (a.out_ld & 3) == 0) {
                  if (a.shift && !a.l2_normalize) v += *reinterpret_cast<const f32x4 *>(a.shift + col);
                  *reinterpret_cast<f32x4 *>(dst + col) = v;
                } else {
#pragma unroll
                  for (int u = 0; u < 4; ++u)
                    if (col + u < a.cout) dst[col + u] = v[u] + ((a.shift && !a.l2_normalize) ? a.shift[col + u] : 0.f);
                }
              } else if (col < a.cout) {
                *reinterpret_cast<f32x4 *>(dst + col) = v;  // y_ld = cout is a multiple of 32 here
              }
            }
          }
        }
      }
    }
    __syncthreads();  // buffer q&1 is free again; buffer (q+1)&1 and the index ring are visible
  }
}

template <int CP, int WM, int WN, int MB, int NB, bool VEC>
static int launch_v2(const ConvKArgs &ka, int64_t tile_bound, int num_cus, hipStream_t stream) {
  constexpr int THREADS = 64 * WM * WN;
  constexpr int CKL = conv_phase_width(CP, MB * NB);
  const size_t lds_bytes = (size_t)2 * DGR_TILE_M * (CKL + 4) * sizeof(float) + 4 * DGR_TILE_M * sizeof(int);
  static int per_cu = 0;
  if (per_cu == 0) {
    const void *kernel = (const void *)sparse_conv_mfma_v2<CP, WM, WN, MB, NB, VEC>;
    DGR_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    int n = 0;
    DGR_CHECK(dgr_resident_blocks(kernel, THREADS, lds_bytes, &n, 1));   // per CU: the context's share sizes the grid
    per_cu = std::min(n, 2048 / THREADS);
  }
  int64_t grid = (int64_t)num_cus * per_cu;
  if (tile_bound < grid) grid = tile_bound;
  grid = (grid + 7) / 8 * 8;
  if (grid < 8) grid = 8;
  sparse_conv_mfma_v2<CP, WM, WN, MB, NB, VEC><<<(int)grid, THREADS, lds_bytes, stream>>>(ka);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// The instantiations that can run.  A layer comes here as K_RULE (net.hip: layer_kind), never as conv1 with <= 8 input
// channels (K_SMALL_CIN / K_CONV1_FUSED: so no cin_pad 8) and never as conv1_tr or final (K_IDENTITY: so no Cin 96, which
// only conv1_tr has).  That leaves the widths of ResUNetBN2C's kernel-map layers (net.hip: LAYERS, CH, TR):
//   32 -> 32 block1;  32 -> 64 conv2;  128 -> 64 conv2_tr;  256 -> 64 conv3_tr            6-D net in every mode
//   64 -> 64 block2, block3_tr, block2_tr;  64 -> 128 conv3;  128 -> 128 block3, block4_tr;  256 -> 128 conv4_tr;
//   128 -> 256 conv4;  256 -> 256 block4            6-D net with DGR_EXACT_F32=1 (else the wide kernel, conv_wide.hip)
//   32 / 64 -> 32  conv1 of a net with 9..32 / 33..64 input channels, zero-padded by make_layer
// and every one of them in a 3-D net that does not run on neighbour tables (more than 8 input channels, or a conv1 size
// above 7), whose K = 27 layers never take the wide kernel.  dgr_debug_conv_layer runs one of the same layers.
// VEC (16-byte gathers) needs Cin and the input's row stride to be multiples of 4.  Every tensor a conv reads has a
// width and a stride out of {32, 64, 96, 128, 256}, except X, the caller's features: conv1 alone reads it, with Cin =
// stride = the caller's width.  So VEC = false is conv1 with 9..64 input channels that are no multiple of 4: the last two rows.
struct RuleConvKernel {
  int cin_pad, cout_pad; bool vec;
  int (*launch)(const ConvKArgs &, int64_t, int, hipStream_t);
  const char *name;
};
#define DGR_V2(CPV, WMV, WNV, MBV, NBV, VECV)                                      \
  {CPV, 32 * WNV * NBV, VECV, launch_v2<CPV, WMV, WNV, MBV, NBV, VECV>,             \
   "sparse_conv_mfma_v2<" #CPV ", " #WMV ", " #WNV ", " #MBV ", " #NBV ", " #VECV ">"}
static const RuleConvKernel RULE_CONV_KERNELS[] = {
    DGR_V2(32, 2, 1, 1, 1, true),   DGR_V2(64, 2, 1, 1, 1, true),
    DGR_V2(32, 2, 2, 1, 1, true),   DGR_V2(64, 2, 2, 1, 1, true),   DGR_V2(128, 2, 2, 1, 1, true), DGR_V2(256, 2, 2, 1, 1, true),
    DGR_V2(64, 1, 4, 2, 1, true),   DGR_V2(128, 1, 4, 2, 1, true),  DGR_V2(256, 1, 4, 2, 1, true),
    DGR_V2(128, 1, 4, 2, 2, true),  DGR_V2(256, 1, 4, 2, 2, true),
    DGR_V2(32, 2, 1, 1, 1, false),  DGR_V2(64, 2, 1, 1, 1, false)};
#undef DGR_V2

int dgr_conv_launch(const DgrConvLaunch &a, int num_cus, hipStream_t stream, const char **kernel_name) {
  DGR_REQUIRE(a.pair_in != nullptr, "sparse conv: no kernel map (kernel-volume-1 convs: dgr_conv_identity_launch)");
  DGR_REQUIRE(a.cin_pad % 8 == 0 && a.cin_pad >= a.cin && a.cin_pad <= 256, "bad cin_pad %d", a.cin_pad);
  const ConvKArgs ka = dgr_conv_kargs(a);
  const int64_t tile_bound = a.tile_bound > 0 ? a.tile_bound : (int64_t)num_cus * 4;
  const bool vec = ((a.cin | a.in_ld) & 3) == 0;
  for (const RuleConvKernel &k : RULE_CONV_KERNELS)
    if (k.cin_pad == a.cin_pad && k.cout_pad == a.cout_pad && k.vec == vec) {
      if (kernel_name) *kernel_name = k.name;
      return k.launch(ka, tile_bound, num_cus, stream);
    }
  dgr_set_error("sparse conv: no kernel instantiation for Cin (padded) %d -> Cout (padded) %d with %s gathers (Cin %d, row stride %d)",
                a.cin_pad, a.cout_pad, vec ? "16-byte" : "element-wise", a.cin, a.in_ld);
  return DGR_EINVAL;
}

// ------------------------------------------------------------------------------------------
// phase 2: out[o, :] = shift (+ residual[o, :]) + sum over the row's pairs (ascending k) of Y[pos, :]
// LPR lanes cooperate on one output row (one float4 column group each); rows are independent.
// ------------------------------------------------------------------------------------------
template <int LPR, bool SPLIT>
__global__ void __launch_bounds__(256)
    reduce_rows_kernel(const float *__restrict__ y, int y_ld, const int32_t *__restrict__ ptr,
                       const int32_t *__restrict__ pos, const int32_t *n_dev, float *__restrict__ out, int out_ld,
                       const float *__restrict__ shift, const float *__restrict__ res, int res_ld, int res_relu,
                       unsigned char *__restrict__ planes, float *__restrict__ scale_out, int out_relu) {
  constexpr int ROWS = 256 / LPR;
  const int n = *n_dev;
  const int sub = threadIdx.x / LPR, c = (threadIdx.x % LPR) * 4;
  for (int64_t row = (int64_t)blockIdx.x * ROWS + sub; row < n; row += (int64_t)gridDim.x * ROWS) {
    f32x4 acc = shift ? *reinterpret_cast<const f32x4 *>(shift + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (res) {
      f32x4 r = *reinterpret_cast<const f32x4 *>(res + row * res_ld + c);
      if (res_relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
      acc += r;
    }
    int j = ptr[row];
    const int end = ptr[row + 1];
    // eight independent product-row loads in flight (their eight slot indices are fetched together first);
    // the additions stay in ascending-k order
    for (; j + 8 <= end; j += 8) {
      int p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = pos[j + u];
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = dgr_y_load<LPR == 64>(y + (int64_t)p[u] * y_ld + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; j + 4 <= end; j += 4) {
      const int p0 = pos[j], p1 = pos[j + 1], p2 = pos[j + 2], p3 = pos[j + 3];
      const f32x4 v0 = dgr_y_load<LPR == 64>(y + (int64_t)p0 * y_ld + c);
      const f32x4 v1 = dgr_y_load<LPR == 64>(y + (int64_t)p1 * y_ld + c);
      const f32x4 v2 = dgr_y_load<LPR == 64>(y + (int64_t)p2 * y_ld + c);
      const f32x4 v3 = dgr_y_load<LPR == 64>(y + (int64_t)p3 * y_ld + c);
      acc += v0; acc += v1; acc += v2; acc += v3;
    }
    for (; j < end; ++j) acc += dgr_y_load<LPR == 64>(y + (int64_t)pos[j] * y_ld + c);
    if (!SPLIT || out) *reinterpret_cast<f32x4 *>(out + row * out_ld + c) = acc;   // (split-only tensors: out == nullptr)
    if constexpr (SPLIT) {
      // the row as the wide-layer kernel gathers it (conv_wide.hip): scale from the row's largest |x| after the
      // consumers' pending ReLU (the LPR lanes of a row are consecutive lanes of one wave), two f16 planes
      const int lo = out_relu ? 0 : (int)0x80000000;
      const i32x4 ab = __builtin_bit_cast(i32x4, acc);   // (bit_cast of a single vector ELEMENT reads element 0)
      const uint32_t mx = dgr_lane_max<LPR>(dgr_abs_max4(ab, lo));
      const float sx = dgr_row_scale_of(mx);
      f16x4 h, m;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        _Float16 hh, mm;
        dgr_split2(__builtin_bit_cast(float, max(ab[u], lo)), sx, hh, mm);   // pending ReLU as one integer max
        h[u] = hh; m[u] = mm;
      }
      // lanes 2 j and 2 j + 1 hold channels 8 j .. 8 j + 3 and 8 j + 4 .. 8 j + 7: they swap one piece, so that the even
      // lane stores 16 bytes of h and the odd lane 16 bytes of m (one 16-byte store per lane instead of two 8-byte ones)
      const bool odd = threadIdx.x & 1;
      const u32x2 hb = __builtin_bit_cast(u32x2, h), mb = __builtin_bit_cast(u32x2, m);
      const u32x2 give = odd ? hb : mb;
      u32x2 got;
      got.x = (uint32_t)__shfl_xor((int)give.x, 1, 64);
      got.y = (uint32_t)__shfl_xor((int)give.y, 1, 64);
      const u32x4 st = odd ? u32x4{got.x, got.y, mb.x, mb.y} : u32x4{hb.x, hb.y, got.x, got.y};
      unsigned char *dst = planes + row * (LPR * 16);
      *reinterpret_cast<u32x4 *>(dst + dgr_split_row_offset(c & ~7, odd ? 1 : 0)) = st;
      if (c == 0) scale_out[row] = sx;
    }
  }
}

int dgr_reduce_rows(const float *y, int cout, const int32_t *ptr, const int32_t *pos, const int32_t *n_dev,
                    int64_t n_cap, float *out, int out_ld, const float *shift, const float *res, int res_ld,
                    int res_relu, hipStream_t stream, const DgrSplitRows *split, int out_relu) {
  DGR_REQUIRE((out_ld & 3) == 0 && (res == nullptr || (res_ld & 3) == 0), "reduce_rows: row strides must be x4");
  DGR_REQUIRE(out || split, "reduce_rows: no output");
  DGR_REQUIRE(!split || (split->planes && split->scale && split->channels == cout && cout % 64 == 0),
              "reduce_rows: split rows need planes, scales and the layer's width (a multiple of 64)");
  const int lpr = cout / 4;
  const int64_t want = std::max<int64_t>(1, dgr_ceil_div(n_cap, 256 / lpr));
  // grid-stride kernels: at most four resident rounds, and a whole number of them
#define DGR_RR1(L, SP)                                                                                         \
  do {                                                                                                         \
    static int resident = 0;                                                                                   \
    if (resident == 0) DGR_CHECK(dgr_resident_blocks((const void *)reduce_rows_kernel<L, SP>, 256, 0, &resident)); \
    const int64_t blocks = want > resident ? (int64_t)resident * std::min<int64_t>(4, want / resident) : want; \
    reduce_rows_kernel<L, SP><<<(int)blocks, 256, 0, stream>>>(y, cout, ptr, pos, n_dev, out, out_ld, shift,   \
                                                               res, res_ld, res_relu, split ? split->planes : nullptr, \
                                                               split ? split->scale : nullptr, out_relu);      \
  } while (0)
#define DGR_RR(L)                       \
  do {                                  \
    if (split) DGR_RR1(L, true);        \
    else DGR_RR1(L, false);             \
  } while (0)
  switch (cout) {
    case 32: DGR_RR1(8, false); break;
    case 64: DGR_RR(16); break;
    case 128: DGR_RR(32); break;
    case 256: DGR_RR(64); break;
    default:
      dgr_set_error("reduce_rows: unsupported width %d", cout);
      return DGR_EINVAL;
  }
#undef DGR_RR1
#undef DGR_RR
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}
