// The two-f16-piece split of f32 operands and the row maximum its scale comes from, shared by every split-operand conv
// kernel (conv_wide.hip, conv_os.hip, and through dense_tile.h conv_dense.hip / conv_up.hip) and by the producers of
// their inputs (reduce_rows in conv.hip, the conv1 epilogues in conv1.hip, the epilogues of conv_os.hip and dense_tile.h, the
// "dense split rows" of conv_dense.hip): one definition, so that a row split by its producer is bit-identical to the
// same row split by a consumer.
#pragma once
#include <stdint.h>

#include "conv_vec.h"

// power of two that moves the largest |x| of a row (given as the integer max of the |x| bit patterns, monotone in the
// magnitude) into [2^14, 2^15); biased exponent clamped to [20, 240]: zero / denormal rows get a finite scale
__device__ __forceinline__ float dgr_row_scale_of(uint32_t max_abs_bits) {
  const uint32_t e = min(max(max_abs_bits >> 23, 20u), 240u);
  return max_abs_bits == 0 ? 1.f : __builtin_bit_cast(float, (268u - e) << 23);
}
// s x = h + m (+ <= 2^-22 |s x|): two f16 pieces by round-to-nearest; sx is a power of two
__device__ __forceinline__ void dgr_split2(float x, float sx, _Float16 &h, _Float16 &m) {
  const float xs = x * sx;
  h = (_Float16)xs;
  m = (_Float16)(xs - (float)h);
}
// dgr_split2 of max(x, relu_lo) for the eight values of two 16-byte chunks (raw bits; relu_lo: the pending ReLU as one
// integer max, 0 or INT_MIN), two values per packed instruction: the same arithmetic as dgr_split2, value by value.
// Dwords 0-1 of the h pieces `hw` and of the m pieces `mw` come from c0, dwords 2-3 from c1.
__device__ __forceinline__ void dgr_split2_x8(i32x4 c0, i32x4 c1, int relu_lo, float sx, i32x4 &hw, i32x4 &mw) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const i32x4 v = h ? c1 : c0;
#pragma unroll
    for (int u = 0; u < 4; u += 2) {
      const f32x2 xs = f32x2{__builtin_bit_cast(float, max(v[u], relu_lo)), __builtin_bit_cast(float, max(v[u + 1], relu_lo))} * sx;
      const f16x2 hh = __builtin_convertvector(xs, f16x2);
      const f16x2 mm = __builtin_convertvector(xs - __builtin_convertvector(hh, f32x2), f16x2);
      hw[2 * h + u / 2] = __builtin_bit_cast(int, hh);
      mw[2 * h + u / 2] = __builtin_bit_cast(int, mm);
    }
  }
}
// |x| as integer bits: monotone in the magnitude, so that a row's largest |x| is an integer (atomic) max
__device__ __forceinline__ uint32_t dgr_abs_bits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
// largest |x| of four values (raw bits, after the pending ReLU) as integer bits: monotone in the magnitude
__device__ __forceinline__ uint32_t dgr_abs_max4(i32x4 b, int relu_lo = (int)0x80000000) {
  return max(max((uint32_t)max(b.x, relu_lo) & 0x7fffffffu, (uint32_t)max(b.y, relu_lo) & 0x7fffffffu),
             max((uint32_t)max(b.z, relu_lo) & 0x7fffffffu, (uint32_t)max(b.w, relu_lo) & 0x7fffffffu));
}
// maximum over a group of W lanes that lie STRIDE apart (both powers of two; every lane gets it): a row's lanes
template <int W, int STRIDE = 1>
__device__ __forceinline__ uint32_t dgr_lane_max(uint32_t mx) {
#pragma unroll
  for (int d = W / 2 * STRIDE; d >= STRIDE; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
  return mx;
}
__device__ __forceinline__ float dgr_inv_pow2(float s) {   // 1 / s for a normal power of two
  return __builtin_bit_cast(float, 0x7f000000u - __builtin_bit_cast(uint32_t, s));
}
// byte offset of channel c (a multiple of 4) of piece p (0 = h, 1 = m) inside a split row (conv_wide.hip: per 64-channel
// block 128 bytes of h, then 128 bytes of m)
__device__ __forceinline__ int dgr_split_row_offset(int c, int p) { return (c >> 6) * 256 + p * 128 + (c & 63) * 2; }
