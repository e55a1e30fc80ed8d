// conv1 of ResUNetBN2C with at most 8 input channels into 32, for gfx950, output-stationary (no product rows):
//   over the rule-major kernel map (dgr_conv_small_cin; 6-D nets, 3-D nets with a conv1 size above 7):
//     conv_cin6_quad_kernel (Cin 6), conv_small_cin_row_kernel (Cin 1), conv_small_cin_kernel (any other Cin);
//   fused with the neighbour search (dgr_conv1_probe; 3-D nets on neighbour tables): the dense-grid builder (grid_*),
//     conv1_grid_mfma (one input channel, ks 3 / 5 / 7), conv1_grid_kernel, and conv1_probe_kernel on the hash table.
#include <algorithm>

#include "dgr_internal.h"
#include "hash.h"
#include "split.h"

// ------------------------------------------------------------------------------------------
// conv1 (Cin <= 8 -> 32): output stationary.  FCGF's first layer has 343 offsets, ~74 neighbours per
// voxel and ONE input channel: as a rule-major GEMM it would write and re-read 260 MB of product rows
// for 0.13 GFLOP.  Here 32 lanes own one output voxel (one channel each), walk its pairs in
// ascending-k order (the same order as the reduction pass, bit-compatible) and write the row once.
// Weights are read in place from the MFMA-tiled layout: W[k][ci][co] sits at
// ((k * 64 + 32 * (ci / 4) + co) * 4 + ci % 4).
// ------------------------------------------------------------------------------------------
// one pair's product for output channel co: the k-ordered fma chain of the MFMA over the input channels
__device__ __forceinline__ float small_cin_pair(const float *__restrict__ in, int in_ld, int in_relu, int cin, int row,
                                                const float *__restrict__ wk, int co) {
  float t = 0.f;
  for (int ci = 0; ci < cin; ++ci) {
    float x = in[(int64_t)row * in_ld + ci];
    if (in_relu) x = fmaxf(x, 0.f);
    t = fmaf(x, wk[(32 * (ci >> 2) + co) * 4 + (ci & 3)], t);
  }
  return t;
}

__global__ void __launch_bounds__(256)
    conv_small_cin_kernel(const float *__restrict__ in, int in_ld, int in_relu, int cin,
                          const float *__restrict__ w, const float *__restrict__ shift,
                          const int32_t *__restrict__ out_ptr, const int32_t *__restrict__ out_pos,
                          const int32_t *__restrict__ pair_in, const uint16_t *__restrict__ pair_k,
                          const int32_t *n_out_dev, float *__restrict__ out, int out_ld) {
  const int n = *n_out_dev;
  const int co = threadIdx.x & 31;
  for (int64_t o = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); o < n; o += (int64_t)gridDim.x * 8) {
    float acc = shift ? shift[co] : 0.f;
    const int end = out_ptr[o + 1];
    int j = out_ptr[o];
    // eight pairs per round: the three dependent index loads (slot -> pair -> input row) of all eight
    // are in flight together; the additions stay in ascending-k order
    for (; j + 8 <= end; j += 8) {
      int pos[8], row[8], kk[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) pos[u] = out_pos[j + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) { row[u] = pair_in[pos[u]]; kk[u] = pair_k[pos[u]]; }
      float y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) y[u] = small_cin_pair(in, in_ld, in_relu, cin, row[u], w + (int64_t)kk[u] * 256, co);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += y[u];
    }
    for (; j < end; ++j) {
      const int pos = out_pos[j];
      acc += small_cin_pair(in, in_ld, in_relu, cin, pair_in[pos], w + (int64_t)pair_k[pos] * 256, co);
    }
    out[o * out_ld + co] = acc;
  }
}

// The same layer with ONE THREAD per output voxel (all 32 output channels in its registers).  The 6-D inlier net's conv1
// has 1.8 pairs per row (the centre offset and, for half the rows, one or two neighbours): with 32 lanes per voxel the
// kernel is 55 k waves that each walk a chain of four dependent loads per pair (row pointer -> slot -> pair -> input
// row / weights), 81 us for 110 k rows; with a thread per voxel it is 1.7 k waves, all resident at once, and the chains
// of 64 voxels run side by side.  Same fma chain per pair, pairs added in ascending-k order: bit-identical results.
template <int CIN>
__global__ void __launch_bounds__(256)
    conv_small_cin_row_kernel(const float *__restrict__ in, int in_ld, int in_relu, const float *__restrict__ w,
                              const float *__restrict__ shift, const int32_t *__restrict__ out_ptr,
                              const int32_t *__restrict__ out_pos, const int32_t *__restrict__ pair_in,
                              const uint16_t *__restrict__ pair_k, const int32_t *n_out_dev, float *__restrict__ out,
                              int out_ld) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= *n_out_dev) return;
  float acc[32];
#pragma unroll
  for (int co = 0; co < 32; ++co) acc[co] = shift ? shift[co] : 0.f;
  const int end = out_ptr[o + 1];
  for (int j = out_ptr[o]; j < end; ++j) {
    const int pos = out_pos[j];
    const int row = pair_in[pos];
    const f32x4 *wk = reinterpret_cast<const f32x4 *>(w + (int64_t)pair_k[pos] * 256);
    float x[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      x[ci] = in[(int64_t)row * in_ld + ci];
      if (in_relu) x[ci] = fmaxf(x[ci], 0.f);
    }
#pragma unroll
    for (int co = 0; co < 32; ++co) {
      // W[k][ci][co] sits at ((k * 64 + 32 * (ci / 4) + co) * 4 + ci % 4): two 16-byte loads per output channel
      const f32x4 w0 = wk[co];
      float t = 0.f;
#pragma unroll
      for (int ci = 0; ci < (CIN < 4 ? CIN : 4); ++ci) t = fmaf(x[ci], w0[ci], t);
      if constexpr (CIN > 4) {
        const f32x4 w1 = wk[32 + co];
#pragma unroll
        for (int ci = 4; ci < CIN; ++ci) t = fmaf(x[ci], w1[ci - 4], t);
      }
      acc[co] += t;
    }
  }
  f32x4 *dst = reinterpret_cast<f32x4 *>(out + o * out_ld);
#pragma unroll
  for (int q = 0; q < 8; ++q) dst[q] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
}

// Cin = 6 (the 'coords' features of the inlier net): a QUAD of lanes per output voxel, lane q of the quad computing output
// channels 8 q .. 8 q + 7.  What the thread-per-voxel kernel above spends its time on is fetching W[k] -- 64 16-byte
// loads per pair and thread, every lane of an instruction at another offset's kilobyte: 64 cache lines per
// instruction through the CU's address path.  Here W[k] is stored quad-major (wq[k][i][q][4], i = 2 ci + half: the four
// lanes of a quad read 64 CONTIGUOUS bytes per instruction, one request), 12 loads per pair and lane.  The fma chain of
// a (pair, output channel) and the order of the pairs are those of the kernel above: bit-identical results.
__global__ void __launch_bounds__(256)
    conv_cin6_quad_kernel(const float *__restrict__ in, int in_ld, int in_relu, const float *__restrict__ wq,
                          const float *__restrict__ shift, const int32_t *__restrict__ out_ptr,
                          const int32_t *__restrict__ out_pos, const int32_t *__restrict__ pair_in,
                          const uint16_t *__restrict__ pair_k, const int32_t *n_out_dev, float *__restrict__ out,
                          int out_ld) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t o = t >> 2;
  const int q = (int)(t & 3);
  if (o >= *n_out_dev) return;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = shift ? shift[8 * q + e] : 0.f;
  const int end = out_ptr[o + 1];
  for (int j = out_ptr[o]; j < end; ++j) {
    const int pos = out_pos[j];
    const int row = pair_in[pos];
    const f32x4 *wk = reinterpret_cast<const f32x4 *>(wq + (int64_t)pair_k[pos] * 192) + q;
    float x[6];
#pragma unroll
    for (int ci = 0; ci < 6; ++ci) {
      x[ci] = in[(int64_t)row * in_ld + ci];
      if (in_relu) x[ci] = fmaxf(x[ci], 0.f);
    }
    float tt[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) tt[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {   // ci = i / 2 ascending: per output channel the chain x0 w0, x1 w1, ... of the kernel above
      const f32x4 wv = wk[4 * i];
#pragma unroll
      for (int e = 0; e < 4; ++e) tt[4 * (i & 1) + e] = fmaf(x[i >> 1], wv[e], tt[4 * (i & 1) + e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += tt[e];
  }
  f32x4 *dst = reinterpret_cast<f32x4 *>(out + o * out_ld + 8 * q);
  dst[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  dst[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

int dgr_conv_small_cin(const float *in, int in_ld, int in_relu, int cin, const float *w_tiled, const float *w_quad,
                       const float *shift, const DgrKernelMap &km, const int32_t *n_out_dev, int64_t n_out_cap, float *out,
                       int out_ld, hipStream_t stream, const char **kernel_name) {
  DGR_REQUIRE(cin >= 1 && cin <= 8, "small-Cin conv: cin=%d", cin);
  const char *name;
  // the inlier net's input widths ('coords' / 'ones' features) have kernels of their own
  if ((out_ld & 3) == 0 && cin == 6) {
    // (make_layer prepares them for every conv1 with six input channels and K > 1; a conv1 on this path has ks = 3 in a
    // 6-D net -- the map builder takes no other -- and ks >= 9 in a 3-D net)
    DGR_REQUIRE(w_quad, "small-Cin conv: six input channels need the quad-major weights");
    name = "conv_cin6_quad_kernel";
    conv_cin6_quad_kernel<<<(int)dgr_ceil_div(n_out_cap * 4, 256), 256, 0, stream>>>(
        in, in_ld, in_relu, w_quad, shift, km.out_ptr, km.out_pos, km.pair_in, km.pair_k, n_out_dev, out, out_ld);
  } else if ((out_ld & 3) == 0 && cin == 1) {
    name = "conv_small_cin_row_kernel";
    conv_small_cin_row_kernel<1><<<(int)dgr_ceil_div(n_out_cap, 256), 256, 0, stream>>>(
        in, in_ld, in_relu, w_tiled, shift, km.out_ptr, km.out_pos, km.pair_in, km.pair_k, n_out_dev, out, out_ld);
  } else {
    name = "conv_small_cin_kernel";
    int64_t blocks = dgr_ceil_div(n_out_cap, 8);
    if (blocks > 16384) blocks = 16384;
    conv_small_cin_kernel<<<(int)blocks, 256, 0, stream>>>(in, in_ld, in_relu, cin, w_tiled, shift, km.out_ptr,
                                                            km.out_pos, km.pair_in, km.pair_k, n_out_dev, out, out_ld);
  }
  DGR_LAUNCH_CHECK();
  if (kernel_name) *kernel_name = name;
  return DGR_OK;
}

// ------------------------------------------------------------------------------------------
// conv1 of the FCGF net fused with its neighbour search (3-D, ks^3 = 343 offsets for 3DMatch, Cin <= 8
// -> 32): the ks^3 kernel map is used by this ONE layer, so building it (343 N probes, a dense hit
// table, ranking, CSR) only to gather ~74 single-channel neighbours per voxel is pure overhead.  Here
// a wave owns one output voxel at a time: its 64 lanes probe 64 offsets at once; the hits are then
// replayed in ascending-k order (ballot + readlane) with lane = output channel accumulating
// x[hit] * W[k][ci][co] -- the same k-ordered sum as the map-based path, bit for bit.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    conv1_probe_kernel(const int32_t *__restrict__ coords, const int32_t *n_dev, const int32_t *__restrict__ table,
                       uint32_t mask, int ks, const float *__restrict__ in, int in_ld, int cin,
                       const float *__restrict__ w, const float *__restrict__ shift, float *__restrict__ out,
                       int out_ld, int32_t *pair_count, const int32_t *skip_flag, uint32_t *__restrict__ out_amax) {
  if (skip_flag && *skip_flag) return;   // the dense-grid kernel did the layer
  const int n = *n_dev;
  const int lane = threadIdx.x & 63;
  const int co = lane & 31;
  const int K = ks * ks * ks, half = ks >> 1;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int pairs = 0;
  for (int64_t o = wave_id; o < n; o += n_waves) {
    const int32_t b = coords[o * 4], x = coords[o * 4 + 1], y = coords[o * 4 + 2], z = coords[o * 4 + 3];
    float acc = shift ? shift[co] : 0.f;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      int hit = -1;
      if (k < K) {
        // offset enumeration: first spatial dimension fastest (same convention as kmap.hip: offset_of)
        int32_t q[4] = {b, x + (k % ks) - half, y + ((k / ks) % ks) - half, z + (k / (ks * ks)) - half};
        hit = dgr_lookup<4>(table, mask, coords, q);
      }
      // every lane fetches the input channels of ITS hit now (lane parallel); the serial replay below
      // then only moves registers (readlane) and reads weights
      // (unconditional clamped loads: a per-lane guard would make the compiler branch and wait per load)
      float xv[8];
      const int64_t hrow = (int64_t)max(hit, 0) * in_ld;
#pragma unroll
      for (int ci = 0; ci < 8; ++ci) {
        xv[ci] = 0.f;
        if (ci < cin) xv[ci] = in[hrow + ci];   // cin is wave-uniform
      }
      unsigned long long live = __ballot(hit >= 0);
      pairs += __popcll(live);
      while (live) {
        const int src = __ffsll((long long)live) - 1;
        live &= live - 1;
        float t = 0.f;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
          if (ci < cin) {
            const float xs = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv[ci]), src));
            const float wv = w[(int64_t)(k0 + src) * 256 + (32 * (ci >> 2) + co) * 4 + (ci & 3)];
            t = fmaf(xs, wv, t);   // same k-ordered fma chain as the MFMA path
          }
        }
        acc += t;
      }
    }
    if (lane < 32) out[o * out_ld + co] = acc;
    if (out_amax) {   // (both half-waves hold the same 32 channels)
      const uint32_t mx = dgr_lane_max<32>(dgr_abs_bits(acc));
      if (lane == 0) atomicMax(out_amax + o, mx);
    }
  }
  if (lane == 0 && pair_count) atomicAdd(pair_count, pairs);
}

// ------------------------------------------------------------------------------------------
// Dense-grid variant of the fused conv1.  A 3-D fragment is compact: the bounding boxes of the batch
// elements (padded by ks/2) hold a few million cells, so the voxel -> row map fits a plain int32 grid
// and a neighbour probe is ONE load of ks consecutive cells per (ky, kz) row -- no hashing, no probe
// chains, 49 independent 28-byte reads per voxel instead of 343 dependent table + key reads.
//   bbox    per-batch-element min / max (block-reduced, 6 atomics per block)
//   layout  grid dims, per-element bases, total cell count; `ok` = fits the cell budget and every batch
//           index is in [0, 64) -- otherwise the hash-probe kernel (launched behind) does the layer
//   clear / fill
//   conv    a wave takes TWO voxels at a time.  Phase A (all lanes, one voxel after the other): lane =
//           (ky, kz) row reads its ks cells; ballots rank the hits in ascending k; (k, row) lists go to
//           LDS.  Phase B: half-wave = voxel, lane = output channel walks its list -- the loads of a step
//           do not depend on the running sum, only the adds are serial -- same k-ordered sum as the
//           map-based path, bit for bit.
// ------------------------------------------------------------------------------------------
constexpr int GRID_MAXB = 64;
struct DgrGridMeta {
  int32_t ok, bad;
  long long total;
  int32_t mn[GRID_MAXB][3], mx[GRID_MAXB][3], dim[GRID_MAXB][3];
  long long base[GRID_MAXB];
};

__global__ void grid_init_kernel(DgrGridMeta *m, int32_t *pair_count) {
  const int b = threadIdx.x;
  if (b == 0) { m->ok = 0; m->bad = 0; m->total = 0; if (pair_count) *pair_count = 0; }
  if (b < GRID_MAXB) {
    for (int d = 0; d < 3; ++d) { m->mn[b][d] = INT32_MAX; m->mx[b][d] = INT32_MIN; m->dim[b][d] = 0; }
    m->base[b] = 0;
  }
}

__global__ void __launch_bounds__(256)
    grid_bbox_kernel(const int32_t *__restrict__ coords, const int32_t *n_dev, DgrGridMeta *m) {
  __shared__ int32_t red[6][256 / 64];
  __shared__ int32_t b0s, mixed;
  const int n = *n_dev;
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if ((int64_t)blockIdx.x * 256 >= n) return;
  const bool live = o < n;
  const int4 c = live ? *reinterpret_cast<const int4 *>(coords + o * 4) : make_int4(0, 0, 0, 0);
  if (threadIdx.x == 0) { b0s = c.x; mixed = 0; }
  __syncthreads();
  if (live && c.x != b0s) mixed = 1;
  if (live && (c.x < 0 || c.x >= GRID_MAXB)) m->bad = 1;
  __syncthreads();
  // min / max of the lanes selected by `mine` over the wave (the others carry the identities)
  auto wave_minmax = [&](bool mine, int32_t (&v)[6]) {
    v[0] = mine ? c.y : INT32_MAX; v[1] = mine ? c.z : INT32_MAX; v[2] = mine ? c.w : INT32_MAX;
    v[3] = mine ? c.y : INT32_MIN; v[4] = mine ? c.z : INT32_MIN; v[5] = mine ? c.w : INT32_MIN;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        v[d] = min(v[d], __shfl_xor(v[d], s, 64));
        v[3 + d] = max(v[3 + d], __shfl_xor(v[3 + d], s, 64));
      }
    }
  };
  int32_t v[6];
  if (mixed) {
    // the block straddles batch elements (a handful of blocks per call): one reduction per wave and batch element
    // present in it, six atomics each.  (Per-thread atomics here -- 1536 on the same few addresses per such block, at
    // ~40 ns each chip-wide -- made this kernel 50 us of the 290-us conv1 layer.)
    const bool ok = live && c.x >= 0 && c.x < GRID_MAXB;
    unsigned long long todo = __ballot(ok);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int b = __shfl(c.x, leader, 64);
      const bool mine = ok && c.x == b;
      wave_minmax(mine, v);
      if ((int)(threadIdx.x & 63) == leader) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { atomicMin(&m->mn[b][d], v[d]); atomicMax(&m->mx[b][d], v[3 + d]); }
      }
      todo &= ~__ballot(mine);
    }
    return;
  }
  wave_minmax(live, v);
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 6; ++d) red[d][threadIdx.x >> 6] = v[d];
  __syncthreads();
  if (threadIdx.x < 6) {
    const int d = threadIdx.x;
    int32_t r = red[d][0];
    for (int w = 1; w < 4; ++w) r = d < 3 ? min(r, red[d][w]) : max(r, red[d][w]);
    const int b = b0s;
    if (b >= 0 && b < GRID_MAXB) {
      if (d < 3) atomicMin(&m->mn[b][d], r); else atomicMax(&m->mx[b][d - 3], r);
    }
  }
}

// one wave: lane b sizes batch element b, a shuffle scan yields the bases (launched with 64 threads = GRID_MAXB)
__global__ void grid_layout_kernel(DgrGridMeta *m, int pad, long long cap) {
  static_assert(GRID_MAXB == 64, "one lane per batch element");
  const int b = threadIdx.x;
  long long vol = 0;
  if (m->mx[b][0] >= m->mn[b][0]) {   // the element has rows
    vol = 1;
    for (int d = 0; d < 3; ++d) {
      const long long e = (long long)m->mx[b][d] - m->mn[b][d] + 1 + 2 * pad;
      m->dim[b][d] = (int32_t)(e < (1ll << 30) ? e : (1ll << 30));
      vol = (vol <= cap && e <= cap) ? vol * e : cap + 1;
    }
  }
  long long incl = vol;   // inclusive scan (every term <= cap + 1: no overflow over 64 lanes)
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const long long up = __shfl_up(incl, s, 64);
    if (b >= s) incl += up;
  }
  m->base[b] = incl - vol;
  const long long total = __shfl(incl, 63, 64);
  if (b == 0) {
    m->total = total <= cap ? total : cap + 1;
    m->ok = (!m->bad && total <= cap) ? 1 : 0;
  }
}

__global__ void grid_clear_kernel(const DgrGridMeta *m, int32_t *__restrict__ cells) {
  if (!m->ok) return;
  const long long total = m->total;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total; i += (long long)gridDim.x * blockDim.x * 4)
    *reinterpret_cast<int4 *>(cells + i) = make_int4(-1, -1, -1, -1);   // capacity is padded to a multiple of 4
}

__device__ __forceinline__ long long grid_cell(const DgrGridMeta *m, int b, int x, int y, int z, int pad) {
  const long long dx = m->dim[b][0], dy = m->dim[b][1];
  return m->base[b] + ((long long)(z - m->mn[b][2] + pad) * dy + (y - m->mn[b][1] + pad)) * dx + (x - m->mn[b][0] + pad);
}

// cells[cell of row o] = o -- or, for a one-channel input (`values`), the row's input value itself: the MFMA kernel then
// needs no second, dependent load per neighbour.  Empty cells hold -1 = 0xffffffff either way (as a float: a NaN
// payload no arithmetic produces; an input feature with exactly these bits would read as "no voxel").
constexpr uint32_t GRID_EMPTY = 0xffffffffu;
__global__ void grid_fill_kernel(const int32_t *__restrict__ coords, const int32_t *n_dev, const DgrGridMeta *m, int pad,
                                 int32_t *__restrict__ cells, const float *__restrict__ values, int values_ld) {
  if (!m->ok) return;
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= *n_dev) return;
  const int4 c = *reinterpret_cast<const int4 *>(coords + o * 4);
  cells[grid_cell(m, c.x, c.y, c.z, c.w, pad)] = values ? __builtin_bit_cast(int32_t, values[o * values_ld]) : (int32_t)o;
}

// what one wave wrote to LDS is visible to all of its lanes behind this (no block barrier: the data is the wave's own)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int C1_MAXK = 343;   // ks <= 7
__global__ void __launch_bounds__(256)
    conv1_grid_kernel(const int32_t *__restrict__ coords, const int32_t *n_dev, const DgrGridMeta *__restrict__ m,
                      const int32_t *__restrict__ cells, int ks, const float *__restrict__ in, int in_ld, int cin,
                      const float *__restrict__ w, const float *__restrict__ shift, float *__restrict__ out,
                      int out_ld, int32_t *pair_count, uint32_t *__restrict__ out_amax) {
  __shared__ int2 lists[256 / 64][2][C1_MAXK + 1];
  if (!m->ok) return;
  const int n = *n_dev;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = ks >> 1, ks2 = ks * ks;
  const int ky = lane % ks, kz = lane / ks;
  const int vsel = lane >> 5, co = lane & 31;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int pairs = 0;
  for (int64_t o0 = wave_id * 2; o0 < n; o0 += n_waves * 2) {
    int nh[2] = {0, 0};
    // ---- phase A: hit lists of the two voxels, ascending k
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int64_t o = o0 + v;
      if (o >= n) break;   // wave-uniform
      const int4 c = *reinterpret_cast<const int4 *>(coords + o * 4);
      int hit[7];
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) hit[kx] = -1;
      if (lane < ks2) {
        const long long c0 = grid_cell(m, c.x, c.y - half, c.z + ky - half, c.w + kz - half, half);
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
          if (kx < ks) hit[kx] = cells[c0 + kx];
      }
      unsigned long long mk[7];
      int before = 0;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        mk[kx] = __ballot(hit[kx] >= 0);
        before += __popcll(mk[kx] & below);
        nh[v] += __popcll(mk[kx]);
      }
      int r = before;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx)
        if (hit[kx] >= 0) lists[wv][v][r++] = make_int2(kx + ks * lane, hit[kx]);
    }
    wave_lds_sync();
    // ---- phase B: half-wave = voxel, lane = output channel
    pairs += nh[0] + nh[1];
    const int my_n = vsel ? nh[1] : nh[0];
    const int trips = max(nh[0], nh[1]);
    float acc = shift ? shift[co] : 0.f;
    // eight list entries per trip: all loads of a trip (per input channel) are issued together -- nothing
    // between them consumes a loaded value -- and only the adds form a serial chain
    for (int r0 = 0; r0 < trips; r0 += 8) {
      int2 e[8];
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        e[u] = (r0 + u < my_n) ? lists[wv][vsel][r0 + u] : make_int2(0, 0);
        t[u] = 0.f;
      }
      for (int ci = 0; ci < cin; ++ci) {   // wave-uniform trip count (1 for FCGF)
        float xs[8], ws[8];
        const int wofs = (32 * (ci >> 2) + co) * 4 + (ci & 3);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          xs[u] = in[(int64_t)e[u].y * in_ld + ci];
          ws[u] = w[(int64_t)e[u].x * 256 + wofs];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = fmaf(xs[u], ws[u], t[u]);   // same k-ordered fma chain as the MFMA path
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = (r0 + u < my_n) ? acc + t[u] : acc;
    }
    const int64_t o = o0 + vsel;
    if (o < n) out[o * out_ld + co] = acc;
    if (out_amax) {   // a voxel's 32 channels are the 32 lanes of a half-wave
      const uint32_t mx = dgr_lane_max<32>(o < n ? dgr_abs_bits(acc) : 0u);
      if (co == 0 && o < n) atomicMax(out_amax + o, mx);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the lists are rewritten by the next pair of voxels
  }
  if (lane == 0 && pair_count) atomicAdd(pair_count, pairs);
}

// ------------------------------------------------------------------------------------------
// The same layer on the matrix cores, for ONE input channel (FCGF: feats = ones [N, 1]): per voxel the layer is a
// 343-term (ks = 7) dot product per output channel, i.e. out[16 voxels x 32 channels] = G[16 x ks^3] . W[ks^3 x 32]
// with G[v][k] = x[neighbour k of v] or 0 -- a GEMM whose left operand is gathered from the dense grid.  A wave owns
// 16 voxels and walks the ks z-slabs of the kernel: lanes = (voxel, y-row) items read their ks consecutive cells of the
// VALUE grid (grid_fill_kernel: the cell holds the voxel's input value, so a neighbour costs no second, dependent load;
// 28 contiguous bytes per item = two vector loads) into a [16 x ks^2] slab of G in LDS, double-buffered per wave (no
// block barrier), and ceil(ks^2 / 4) x 2 v_mfma_f32_16x16x4_f32 multiply it with the slab's weights.  Zeros of G
// contribute exactly 0 to the fma chain, so a channel's value is the ascending-k chain over the hits, as in the scalar
// kernels (one rounding per term instead of two).
// Weights: wt[kz][s][lane] = {W[k][lane & 15], W[k][16 + (lane & 15)]} with k = kz ks^2 + 4 s + (lane >> 4) (zero past
// the slab): the A operands of step s as ONE coalesced 8-byte load per lane (net.hip); operands are swapped
// (D = W^T G^T): a lane ends with one voxel and 4 consecutive channels per 16-channel block.
// Round 3 kept row indices in the grid: per item 7 index loads + 7 dependent value loads, every lane on its own cache
// line -- 196 scattered load instructions per 16 voxels, 213 us for 195 k voxels, bound by the address path.
// ------------------------------------------------------------------------------------------
template <int KS>
__global__ void __launch_bounds__(256)
    conv1_grid_mfma(const int32_t *__restrict__ coords, const int32_t *n_dev, const DgrGridMeta *__restrict__ m,
                    const int32_t *__restrict__ cells, const float *__restrict__ wt, const float *__restrict__ shift,
                    float *__restrict__ out, int out_ld, int32_t *pair_count, uint32_t *__restrict__ out_amax) {
  constexpr int KS2 = KS * KS, HALF = KS / 2;
  constexpr int RS = (KS2 + 3) / 4 * 4;          // slab length padded to MFMA k-steps
  constexpr int LDG = RS + 1;
  constexpr int ITEMS = 16 * KS;                 // (voxel, y-row) items per slab
  constexpr int ROUNDS = (ITEMS + 63) / 64;
  __shared__ float G[4][2][16][LDG];
  __shared__ int4 vc[4][16];
  __shared__ int pair_sum;
  if (!m->ok) return;
  const int n = *n_dev;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t v0 = ((int64_t)blockIdx.x * 4 + wv) * 16;
  if (threadIdx.x == 0) pair_sum = 0;
  __syncthreads();
  int pairs = 0;
  if (v0 < n) {
    if (lane < 16) vc[wv][lane] = v0 + lane < n ? *reinterpret_cast<const int4 *>(coords + (v0 + lane) * 4) : make_int4(-1, 0, 0, 0);
    // the padding columns stay zero for the whole kernel
    for (int e = lane; e < 2 * 16 * (LDG - KS2); e += 64) {
      const int b = e / (16 * (LDG - KS2)), r = (e / (LDG - KS2)) % 16, c = KS2 + e % (LDG - KS2);
      G[wv][b][r][c] = 0.f;
    }
    wave_lds_sync();
    uint32_t cell[ROUNDS][KS];
    // request the grid cells of slab kz for this lane's items (dead items read cell 0 of the grid: no branch)
    auto cells_of = [&](int kz) {
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        const int it = lane + 64 * r;
        const int v = it / KS, ky = it % KS;
        const int4 c = vc[wv][min(v, 15)];
        const bool live = it < ITEMS && c.x >= 0;
        const long long c0 = live ? grid_cell(m, c.x, c.y - HALF, c.z + ky - HALF, c.w + kz - HALF, HALF) : 0;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) cell[r][kx] = (uint32_t)cells[c0 + kx];
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) cell[r][kx] = live ? cell[r][kx] : GRID_EMPTY;
      }
    };
    // the landed values -> slab buffer b
    auto fill = [&](int b) {
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        const int it = lane + 64 * r;
        const int v = it / KS, ky = it % KS;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const bool hit = cell[r][kx] != GRID_EMPTY;
          pairs += hit;
          if (it < ITEMS) G[wv][b][v][kx + KS * ky] = hit ? __builtin_bit_cast(float, cell[r][kx]) : 0.f;
        }
      }
    };
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    cells_of(0);
    fill(0);
    for (int kz = 0; kz < KS; ++kz) {
      if (kz + 1 < KS) cells_of(kz + 1);          // in flight while this slab is multiplied
      wave_lds_sync();
      const float *g = &G[wv][kz & 1][lane & 15][lane >> 4];
      const f32x2 *w = reinterpret_cast<const f32x2 *>(wt) + (int64_t)kz * (RS / 4) * 64 + lane;
#pragma unroll
      for (int s = 0; s < RS / 4; ++s) {
        const float b = g[4 * s];
        const f32x2 a = w[s * 64];
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b, acc[1], 0, 0, 0);
      }
      if (kz + 1 < KS) fill((kz + 1) & 1);
    }
    const int64_t o = v0 + (lane & 15);
    uint32_t mx = 0;
    if (o < n) {
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        f32x4 v = acc[jb];
        if (shift) v += *reinterpret_cast<const f32x4 *>(shift + 16 * jb + 4 * (lane >> 4));
        *reinterpret_cast<f32x4 *>(out + o * out_ld + 16 * jb + 4 * (lane >> 4)) = v;
        mx = max(mx, dgr_abs_max4(__builtin_bit_cast(i32x4, v)));
      }
    }
    if (out_amax) {   // the row's largest |x| for its split-operand consumers (conv_os.hip / conv_dense.hip): a voxel's
                      // channels sit in the four lanes (lane & 15) + 16 q
      mx = dgr_lane_max<4, 16>(mx);
      if (lane < 16 && o < n) atomicMax(out_amax + o, mx);
    }
  }
  if (pair_count) {   // (statistics: one atomic per workgroup)
    for (int d = 32; d > 0; d >>= 1) pairs += __shfl_down(pairs, d, 64);
    if (lane == 0 && pairs) atomicAdd(&pair_sum, pairs);
    __syncthreads();
    if (threadIdx.x == 0 && pair_sum) atomicAdd(pair_count, pair_sum);
  }
}

int dgr_conv1_probe(DgrArena &arena, const DgrCoordMap &cm, int ks, const float *in, int in_ld, int cin,
                    const float *w_tiled, const float *shift, float *out, int out_ld, int32_t *pair_count,
                    hipStream_t stream, const float *w_compact, const char **kernel_name, uint32_t *out_amax) {
  DGR_REQUIRE(cin >= 1 && cin <= 8 && ks % 2 == 1, "conv1 probe: cin=%d ks=%d", cin, ks);
  if (pair_count && ks > 7) DGR_HIP_CHECK(hipMemsetAsync(pair_count, 0, sizeof(int32_t), stream));   // (else: grid_init_kernel)
  const int32_t *grid_done = nullptr;
  if (ks <= 7) {
    // dense grid: up to 64 M cells (256 MB) of transient arena memory
    static const long long cap = 64ll << 20;
    DgrArena::Mark mk = arena.mark();
    DgrGridMeta *meta;
    int32_t *cells;
    DGR_ALLOC(meta, arena, DgrGridMeta, 1);
    DGR_ALLOC(cells, arena, int32_t, cap + 4);
    grid_init_kernel<<<1, 64, 0, stream>>>(meta, pair_count);
    grid_bbox_kernel<<<(int)dgr_ceil_div(cm.n_cap, 256), 256, 0, stream>>>(cm.coords, cm.n_dev, meta);
    grid_layout_kernel<<<1, 64, 0, stream>>>(meta, ks >> 1, cap);
    grid_clear_kernel<<<2048, 256, 0, stream>>>(meta, cells);
    // one input channel + MFMA-tiled weights: the grid holds the input VALUES and conv1_grid_mfma does the layer
    const bool mfma = cin == 1 && w_compact && (out_ld & 3) == 0 && (ks == 3 || ks == 5 || ks == 7);
    grid_fill_kernel<<<(int)dgr_ceil_div(cm.n_cap, 256), 256, 0, stream>>>(cm.coords, cm.n_dev, meta, ks >> 1, cells,
                                                                           mfma ? in : nullptr, in_ld);
    if (mfma) {
      const int wgs = (int)dgr_ceil_div(cm.n_cap, 64);
#define DGR_C1(KSV)                                                                                                      \
  case KSV:                                                                                                              \
    conv1_grid_mfma<KSV><<<wgs, 256, 0, stream>>>(cm.coords, cm.n_dev, meta, cells, w_compact, shift, out, out_ld, pair_count, out_amax); \
    if (kernel_name) *kernel_name = "conv1_grid_mfma<" #KSV ">";                                                         \
    break;
      switch (ks) { DGR_C1(3) DGR_C1(5) DGR_C1(7) }
#undef DGR_C1
    } else {
      // grid-stride kernel: a whole number of resident rounds (a ragged last round costs up to 10 %)
      static int resident = 0;
      if (resident == 0) DGR_CHECK(dgr_resident_blocks((const void *)conv1_grid_kernel, 256, 0, &resident));
      int64_t blocks = dgr_ceil_div(cm.n_cap, 8);
      if (blocks > resident) blocks = (int64_t)resident * std::min<int64_t>(4, blocks / resident);
      conv1_grid_kernel<<<(int)blocks, 256, 0, stream>>>(cm.coords, cm.n_dev, meta, cells, ks, in, in_ld, cin, w_tiled, shift,
                                                         out, out_ld, pair_count, out_amax);
      if (kernel_name) *kernel_name = "conv1_grid_kernel";
    }
    DGR_LAUNCH_CHECK();
    grid_done = &meta->ok;
    arena.rewind(mk);   // stream order keeps the grid alive until the kernels above are done
  }
  {
    // (grid-stride; it returns at once when the dense-grid kernel did the layer: a modest grid keeps that case cheap)
    int64_t blocks = dgr_ceil_div(cm.n_cap, 4);
    if (blocks > 4096) blocks = 4096;
    conv1_probe_kernel<<<(int)blocks, 256, 0, stream>>>(cm.coords, cm.n_dev, cm.table, cm.table_mask, ks, in, in_ld, cin,
                                                        w_tiled, shift, out, out_ld, pair_count, grid_done, out_amax);
  }
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}
