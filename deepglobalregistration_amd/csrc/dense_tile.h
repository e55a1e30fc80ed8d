// The shared body of the two dense-tile kernels, sparse_conv_dense_f16x2 (conv_dense.hip) and sparse_conv_up_f16x2
// (conv_up.hip): the ONE quad-coalesced gather, the ONE operand build (split of split.h, ds_bpermute into MFMA B-operand
// order; the row's scale and fold stay in the kernels, see there), the three-product MFMA step and the output-row epilogue, as __forceinline__ pieces that take
// the tile shape as template parameters, and the common part of the kernels' arguments with its host-side checks.
// What stays in each kernel is what differs: block scheduling, the weight ring's index mapping, the loop nest with
// the place where `tmp` is zeroed and folded, and every scheduling barrier between these pieces.
//
// RG = 16-row groups per wave, S = 32-channel steps of the gathered row part (at most 64 channels: S <= 2).
#pragma once
#include "dgr_internal.h"
#include "split.h"

// ---- arguments both kernels take, filled from the layer's launch record
struct DenseTileArgs {
  const float *in;
  float *out;
  const float *shift;
  const u32x4 *wb;            // split weights in the dense-tile operand order (net.hip): two f16 pieces, each
                              // [27][Cin / 32][Cout / 16][64] x 16 bytes
  int64_t piece_stride;       // 16-byte units per piece
  const int32_t *nbr;
  int64_t n_pad;
  int in_ld, in_relu, out_ld, out_relu;
  float w_unscale;            // inverse of the layer's weight scale
  uint32_t in_bytes;          // size of the input tensor (row capacity x row stride): bound of the buffer loads
  const uint32_t *row_amax;   // bits of every input row's largest |x| after the pending ReLU (from the row's producer)
  uint32_t *out_amax, *out_amax2;   // (nullable) the same for the rows written here: atomicMax per row
  // (The order of the fields is part of the generated code: it decides which kernel arguments one scalar load fetches
  // together, and with that how the compiler schedules the weight ring's index arithmetic between the MFMAs of
  // conv_up.hip.  With this order every loop is the one measured before the record was shared; with w_unscale and
  // in_bytes last, conv_up's is not.  profiles/dense_tile_refactor_resources.txt.)
};

// fills the common arguments and makes the checks both kernels need; `what` prefixes the messages
static inline int dgr_dense_tile_args(DenseTileArgs &ka, const DgrConvOsLaunch &a, const char *what) {
  DGR_REQUIRE(a.wbd && a.row_amax, "%s: needs the split weights in the dense-tile operand order and the input rows' maxima", what);
  DGR_REQUIRE((a.in_ld & 3) == 0 && (a.out_ld & 3) == 0 && (a.res == nullptr || (a.res_ld & 3) == 0),
              "%s: row strides must be multiples of 4", what);
  DGR_REQUIRE(a.n_in_cap > 0 && dgr_fits_32bit_offsets(a.n_in_cap, a.in_ld), "%s: input tensor beyond 2 GB", what);
  ka.in = a.in; ka.out = a.out; ka.shift = a.shift;
  ka.wb = static_cast<const u32x4 *>(a.wbd); ka.piece_stride = a.piece_stride;
  ka.nbr = a.nbr->nbr; ka.n_pad = a.nbr->n_pad;
  ka.in_ld = a.in_ld; ka.in_relu = a.in_relu; ka.out_ld = a.out_ld; ka.out_relu = a.out_relu;
  ka.row_amax = a.row_amax; ka.out_amax = a.out_amax; ka.out_amax2 = a.out_amax2;
  ka.w_unscale = a.w_unscale;
  ka.in_bytes = (uint32_t)(a.n_in_cap * (int64_t)a.in_ld * 4);
  return DGR_OK;
}

// the gathered rows of one loop step (raw bits, requested one step ahead), their maxima and table entries
template <int RG, int S>
struct DenseTileRows { f32x4 raw[RG][S][2]; uint32_t mx[RG]; int nv[RG]; };

// Request layout: lane L = 4 r + c reads 16 bytes of row r of the group so that every QUAD of lanes reads 64
// contiguous bytes of one row -- one request of the vector-memory path per quad.  (Requesting straight in MFMA
// operand layout, lane = 16 chunk + row, makes every lane of a quad touch a different row: four requests per quad,
// measured 64 cycles per instruction and the kernel bounded by nothing else.)  The operand layout is restored after
// the split by ds_bpermute (the LDS crossbar, no LDS memory).
// nbr_of(rg) = this lane's table entry of row group rg, i.e. of its row 16 rg + (lane >> 2) (the kernel's LDS table,
// read there, where the compiler knows its address space); col_bytes = byte offset of the gathered part inside a row.
// PS: "dense split rows" (conv_dense.hip) -- a row is its h plane, then its m plane, 64 S bytes each, and a request
// takes chunk (lane & 3) of a 32-channel group from either.
// (The scalars come by reference, as the lambda this function replaces captured them: with `lane` by value the compiler
// orders the requests of the offset loop differently and moves a wait for them half an offset forward,
// profiles/dense_tile_refactor_resources.txt.)
template <int RG, int S, bool PS, class NbrOf>
__device__ __forceinline__ void dense_tile_request(DenseTileRows<RG, S> &g, const NbrOf &nbr_of, const int &lane,
                                                   const __amdgpu_buffer_rsrc_t &in_rsrc, const DenseTileArgs &a,
                                                   uint32_t col_bytes) {
  // unconditional requests: no branches in the loop body, so that the requests stay where they are written
  // (conv_os.hip, same reason)
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const int n = nbr_of(rg);
    const int ne = max(n, 0);
    // buffer loads: a missing neighbour gets an offset past the tensor -- the bounds check returns zeros without a
    // memory access, and the request stays branch-free
    const uint32_t off = n >= 0 ? (uint32_t)n * (uint32_t)((PS ? 32 * S : a.in_ld) * 4) + col_bytes + 16u * (lane & 3) : a.in_bytes;
    const uint32_t mv = a.row_amax[ne];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if constexpr (PS) {
        g.raw[rg][s][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off + 64 * s, 0, 0));
        g.raw[rg][s][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off + 64 * S + 64 * s, 0, 0));
      } else {
        g.raw[rg][s][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off + 128 * s, 0, 0));
        g.raw[rg][s][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off + 128 * s + 64, 0, 0));
      }
    }
    g.mx[rg] = mv;   // (turned into the scale, and selected against `nv`, when it is consumed: nothing here may wait for the request)
    g.nv[rg] = n;
  }
}

// One B operand pair: the two 16-byte chunks a lane requested of one row and 32-channel step, as s x = h + m, two f16
// pieces (dgr_split2_x8 with the row's scale `sx`; under PS the chunks ARE the ready-made pieces), brought into MFMA B
// layout: lane T = 16 lq + lr of the operand layout takes from lane 4 lr + lq of the request layout,
// from = 4 (4 (lane & 15) + (lane >> 4)).
// (The row's scale and `fold` stay typed out in both kernels, five lines each: with them in here -- per loop step or
// per row group, scalars by value or by reference -- conv_up.hip's loop comes out with 212 instead of 211 VGPRs or with
// the fold's permute in another place, profiles/dense_tile_refactor_resources.txt.)
template <bool PS>
__device__ __forceinline__ void dense_tile_operand(f32x4 c0, f32x4 c1, int from, int relu_lo, float sx, f16x8 &bh, f16x8 &bm) {
  i32x4 hw, mw;   // four dwords = eight halves each: elements 0..3 from the first request, 4..7 from the second
  if constexpr (PS) {
    hw = __builtin_bit_cast(i32x4, c0);
    mw = __builtin_bit_cast(i32x4, c1);
  } else {
    dgr_split2_x8(__builtin_bit_cast(i32x4, c0), __builtin_bit_cast(i32x4, c1), relu_lo, sx, hw, mw);
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    hw[d] = __builtin_amdgcn_ds_bpermute(from, hw[d]);
    mw[d] = __builtin_amdgcn_ds_bpermute(from, mw[d]);
  }
  bh = __builtin_bit_cast(f16x8, hw);
  bm = __builtin_bit_cast(f16x8, mw);
}

// One 32-channel step of one 16-column block for every row group: tmp += w_m x_h + w_h x_m + w_h x_h, in this order
// (it fixes the rounding of the f32 sums)
template <int RG, int S>
__device__ __forceinline__ void dense_tile_mfma(f32x4 (&tmp)[RG], f16x8 wh, f16x8 wm, const f16x8 (&bh)[RG][S],
                                                const f16x8 (&bm)[RG][S], int s) {
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) tmp[rg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wm, bh[rg][s], tmp[rg], 0, 0, 0);
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) tmp[rg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bm[rg][s], tmp[rg], 0, 0, 0);
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) tmp[rg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bh[rg][s], tmp[rg], 0, 0, 0);
}

// One output row of NCB 16-column blocks, its channels 16 cb + 4 lq .. + 3 in the four lanes lr + 16 lq of the wave:
// ReLU applied when the tensor carries one (`total` keeps the clamped values), stored once (`out` = this lane's first
// channel of row 0, or null for a tensor nobody reads as f32), and, with `want_max` (kernel-uniform), the row's
// largest |x| left behind for the split-operand consumers of the tensor.  `row` < 0: no such row.  Returns the maximum.
template <int NCB>
__device__ __forceinline__ uint32_t dense_tile_store_row(f32x4 (&total)[NCB], int64_t row, float *out, int out_ld, int out_relu, int lq,
                                                         bool want_max, uint32_t *out_amax, uint32_t *out_amax2) {
  const float out_lo = out_relu ? 0.f : -__builtin_inff();
  uint32_t mx = 0;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    f32x4 v = total[cb];
    v.x = fmaxf(v.x, out_lo); v.y = fmaxf(v.y, out_lo); v.z = fmaxf(v.z, out_lo); v.w = fmaxf(v.w, out_lo);
    total[cb] = v;
    if (row >= 0) {
      if (out) *reinterpret_cast<f32x4 *>(out + row * out_ld + 16 * cb) = v;
      mx = max(mx, dgr_abs_max4(__builtin_bit_cast(i32x4, v)));
    }
  }
  if (want_max) {
    mx = dgr_lane_max<4, 16>(mx);
    if (lq == 0 && row >= 0) {
      if (out_amax) atomicMax(out_amax + row, mx);
      if (out_amax2) atomicMax(out_amax2 + row, mx);
    }
  }
  return mx;
}
