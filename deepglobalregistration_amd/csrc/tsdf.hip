// TSDF fusion of the depth frames of one fragment (the reference's util/integration.py: an Open3D ScalableTSDFVolume fed
// 50 frames, then the surface): depth frames + camera poses in, the zero crossings of the fused truncated signed distance
// on the voxel lattice's edges out -- the positions marching cubes gives its vertices.  include/dgr_hip.h at
// dgr_tsdf_fragment states the arithmetic in full; tests/tsdf_ref.py is the same statement in numpy.
//
// Passes:
//   ts_depth_lut   d = raw / depth_scale for the 65536 raw values, -1 where the pixel is invalid (one division per VALUE)
//   ts_multiplier  m[v][u] = sqrt((1 + ((u - cx)/fx)^2) + ((v - cy)/fy)^2), the ray length per unit depth, once per call
//   ts_candidates  one thread per strided pixel: back-project, pose, the 2 x 2 x 2 blocks its truncation band touches
//   unique rows    dgr_unique_rows over the 3-int keys, dropped candidates skipped: a slot of the hash keeps the SMALLEST
//                  candidate of a key, flag = "I am that candidate", scan -> the block's place in the list
//   ts_blocks      the flagged candidates write the block list                       -- host sync 1: nb
//   ts_integrate   ONE WORKGROUP PER BLOCK (four per 16^3 block, a slab of z-layers each), voxel-stationary: a thread keeps
//                  tsdf / weight (with colour: and the three integer colour sums) of its voxels in registers over the whole
//                  frame loop and stores them once
//   ts_extract<0>  the same workgroups: crossings per workgroup; scan -> a workgroup's first point -- host sync 2: P
//   ts_extract<1>  the same pass again, writing (with colour: the point's colour beside its position)
//
// Determinism: a voxel is owned by one thread, frames are applied in order, output positions come from scans -- no
// floating-point atomics, and the only integer atomics (hash insertion, a statistics counter) are order-free.
#include "dgr_internal.h"
#include "hash.h"
#include "scan.h"
#include "tsdf_common.h"

#include <cmath>
#include <cstring>

constexpr int TS_THREADS = 256;
constexpr double TS_BLOCK_LIMIT = (double)DGR_TSDF_BLOCK_LIMIT;

struct TsCam {
  double fx, fy, cx, cy;
  double voxel, trunc, bl, depth_trunc;
  int F, H, W, Hs, Ws, stride;
};

__global__ void __launch_bounds__(TS_THREADS) ts_depth_lut(double depth_scale, double depth_trunc, double *__restrict__ dlut) {
#pragma clang fp contract(off)
  const int raw = blockIdx.x * TS_THREADS + threadIdx.x;
  if (raw >= 65536) return;
  const double d = (double)raw / depth_scale;
  dlut[raw] = (raw > 0 && d <= depth_trunc) ? d : -1.0;
}

__global__ void __launch_bounds__(TS_THREADS) ts_multiplier(TsCam cam, double *__restrict__ mtab) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (i >= (int64_t)cam.H * cam.W) return;
  const int u = (int)(i % cam.W), v = (int)(i / cam.W);
  const double xn = ((double)u - cam.cx) / cam.fx, yn = ((double)v - cam.cy) / cam.fy;
  const double xx = xn * xn, yy = yn * yn;
  mtab[i] = sqrt((1.0 + xx) + yy);
}

// candidate row s * 8 + corner of strided pixel s = (f Hs + vs) Ws + us; bit a of the corner selects hi over lo on axis a.
// A corner that repeats an earlier corner of its own pixel (lo == hi on an axis whose bit is set), or the same corner of the
// pixel before it (neighbouring pixels mostly share their blocks), is dropped: the repeated candidate has the smaller
// number and is itself either kept or a repeat of a still smaller one, so the first occurrence of every key is among
// the kept rows -- and most rows never reach the hash.
__global__ void __launch_bounds__(TS_THREADS)
    ts_candidates(const uint16_t *__restrict__ depth, const double *__restrict__ dlut, const double *__restrict__ pose, TsCam cam,
                  int64_t ns, int32_t *__restrict__ keys, int32_t *__restrict__ row_first) {
#pragma clang fp contract(off)
  const int64_t s = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (s >= ns) return;
  const int us = (int)(s % cam.Ws), vs = (int)((s / cam.Ws) % cam.Hs), f = (int)(s / ((int64_t)cam.Ws * cam.Hs));
  const int u = us * cam.stride, v = vs * cam.stride;
  const double d = dlut[depth[((int64_t)f * cam.H + v) * cam.W + u]];
  bool valid = d >= 0.0;
  const double dd = valid ? d : 0.0;
  const double x = (((double)u - cam.cx) / cam.fx) * dd, y = (((double)v - cam.cy) / cam.fy) * dd, z = dd;
  const double *M = pose + (int64_t)f * 12;
  double lo[3], hi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double p = ((M[r * 4] * x + M[r * 4 + 1] * y) + M[r * 4 + 2] * z) + M[r * 4 + 3];
    lo[r] = floor((p - cam.trunc) / cam.bl);
    hi[r] = floor((p + cam.trunc) / cam.bl);
    if (!(lo[r] >= -TS_BLOCK_LIMIT && hi[r] < TS_BLOCK_LIMIT)) valid = false;
  }
  int32_t ilo[3], ihi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    ilo[r] = valid ? (int32_t)lo[r] : 0;
    ihi[r] = valid ? (int32_t)hi[r] : 0;
  }
  // the pixel before (the lane below: active whenever this one is, its candidates all numbered lower)
  int32_t plo[3], phi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    plo[r] = __shfl_up(ilo[r], 1);
    phi[r] = __shfl_up(ihi[r], 1);
  }
  const bool pvalid = __shfl_up((int)valid, 1) && (threadIdx.x & 63) != 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t row = s * 8 + c;
    bool dup = false, same = pvalid;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const bool up = (c >> a) & 1;
      const int32_t k = up ? ihi[a] : ilo[a];
      keys[row * 3 + a] = k;
      dup |= up && ihi[a] == ilo[a];
      same &= k == (up ? phi[a] : plo[a]);
    }
    row_first[row] = (valid && !dup && !same) ? DGR_ROW_PENDING : DGR_ROW_DROPPED;
  }
}

__global__ void __launch_bounds__(TS_THREADS)
    ts_blocks(const int32_t *__restrict__ keys, const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n,
              int64_t nb, int32_t *__restrict__ bkeys) {
  const int64_t r = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (r >= n || !flag[r]) return;
  const int64_t k = rank[r];
  if (k >= nb) return;   // (cannot happen: nb IS the number of flags; keeps the store inside the array whatever happens)
#pragma unroll
  for (int a = 0; a < 3; ++a) bkeys[k * 3 + a] = keys[r * 3 + a];
}

// Voxel-stationary integration.  Thread t owns the voxels l = t + 256 k of its workgroup's slab: the same (lx, ly) and
// several lz, so
// E0 x + E1 y of a row is formed once per frame and thread and shared by its voxels (the product and the sum have the
// bits they have wherever they are computed; nothing is stepped incrementally).  The 12 extrinsic doubles of a frame and
// the intrinsics are the same for the whole wave.
// Cull: per chunk of 256 frames, thread t decides for frame t whether ANY voxel centre of the block can be updated: the
// centres lie in a ball of radius sqrt(3)/2 bl around the block's centre, and an update needs z > 0, z < depth_trunc +
// sdf_trunc (sdf > -trunc with m >= 1 and d <= depth_trunc) and a projection inside the image, i.e. the centre on the inner
// side of the four planes through the camera that bound [0, W) x [0, H) in (uf, vf).  The test runs in camera coordinates,
// where the ball's image lies within (largest row norm of the extrinsic's 3x3 part) x the world radius of the centre's image:
// the radius term is stretched by max(1, that norm) -- 1 for a rigid pose, whatever an accepted pose that scales or shears
// needs.  A frame is skipped only if the ball
// lies outside one of these half-spaces by a margin of 1 % of the radius + 1e-6 + 1e-9 |centre|, orders of magnitude above
// the rounding of either side; the bitwise comparison with the uncalled statement is the proof that nothing is lost.
// workgroups per block: TsdfSplit (tsdf_common.h)
// COLOR (compile time; without it the kernel is the depth-only one, untouched by the rest): every update also adds the
// pixel's colour, three byte loads from the caller's uint8 [F,H,W,3], to the voxel's three int32 sums, kept in registers
// like tsdf / weight.  (Measured against one 32-bit load per update from words packed by a pre-pass: DESIGN.md 4.10.)  The
// sums leave through LDS, so that a store instruction writes 256 consecutive words of the [voxel][3] layout.
template <int B, bool COLOR>
__global__ void __launch_bounds__(TS_THREADS)
    ts_integrate(const int32_t *__restrict__ bkeys, const uint16_t *__restrict__ depth, const double *__restrict__ dlut,
                 const double *__restrict__ mtab, const double *__restrict__ ext, TsCam cam, float *__restrict__ tsdf_out,
                 int32_t *__restrict__ weight_out, unsigned long long *kept, const uint8_t *__restrict__ color,
                 int32_t *__restrict__ rgb_out) {
#pragma clang fp contract(off)
  constexpr int SPLIT = TsdfSplit<B>::value, PART = B * B * B / SPLIT;
  constexpr int V = B * B * B, VPT = PART / TS_THREADS, ZSTEP = TS_THREADS / (B * B);
  __shared__ unsigned char keep[TS_THREADS];
  __shared__ int32_t stage[COLOR ? VPT * TS_THREADS * 3 : 1];
  int32_t rgb[COLOR ? VPT : 1][3];
  if constexpr (COLOR) {
#pragma unroll
    for (int k = 0; k < VPT; ++k) rgb[k][0] = rgb[k][1] = rgb[k][2] = 0;
  }
  const int b = blockIdx.x / SPLIT, part = blockIdx.x % SPLIT, t = threadIdx.x;
  const int bx = bkeys[(int64_t)b * 3], by = bkeys[(int64_t)b * 3 + 1], bz = bkeys[(int64_t)b * 3 + 2];
  const int lx = t % B, ly = (t / B) % B, lz0 = part * (B / SPLIT) + t / (B * B);
  const double x = ((double)(bx * B + lx) + 0.5) * cam.voxel, y = ((double)(by * B + ly) + 0.5) * cam.voxel;
  double z[VPT];
  float tsdf[VPT];
  int32_t weight[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    z[k] = ((double)(bz * B + lz0 + k * ZSTEP) + 0.5) * cam.voxel;
    tsdf[k] = 0.f;
    weight[k] = 0;
  }
  const double Wd = (double)cam.W, Hd = (double)cam.H;
  // the cull's ball (any arithmetic will do here: the margin pays for it)
  const double ccx = ((double)bx + 0.5) * cam.bl, ccy = ((double)by + 0.5) * cam.bl, ccz = ((double)bz + 0.5) * cam.bl;
  const double rad = 0.8660254037844387 * cam.bl;
  const double margin = rad * 1.01 + 1e-6 + 1e-9 * (fabs(ccx) + fabs(ccy) + fabs(ccz));
  unsigned nkept = 0;
  for (int base = 0; base < cam.F; base += TS_THREADS) {
    __syncthreads();
    {
      const int f = base + t;
      bool k = false;
      if (f < cam.F) {
        const double *E = ext + (int64_t)f * 12;
        const double px = E[0] * ccx + E[1] * ccy + E[2] * ccz + E[3];
        const double py = E[4] * ccx + E[5] * ccy + E[6] * ccz + E[7];
        const double pz = E[8] * ccx + E[9] * ccy + E[10] * ccz + E[11];
        // the ball in camera coordinates: coordinate r of E (c' - c) is at most |row r of E's 3x3 part| |c' - c|
        const double n0 = E[0] * E[0] + E[1] * E[1] + E[2] * E[2], n1 = E[4] * E[4] + E[5] * E[5] + E[6] * E[6];
        const double n2 = E[8] * E[8] + E[9] * E[9] + E[10] * E[10];
        const double stretch = fmax(1.0, sqrt(fmax(fmax(n0, n1), n2)));
        const double mg = margin * stretch + 1e-9 * (fabs(px) + fabs(py) + fabs(pz));
        const double l = cam.cx + 0.5, rr = Wd - cam.cx - 0.5, tt = cam.cy + 0.5, bb = Hd - cam.cy - 0.5;
        k = pz > -mg && pz - mg < cam.depth_trunc + cam.trunc
            && cam.fx * px + l * pz >= -mg * (cam.fx + fabs(l)) && cam.fx * px - rr * pz <= mg * (cam.fx + fabs(rr))
            && cam.fy * py + tt * pz >= -mg * (cam.fy + fabs(tt)) && cam.fy * py - bb * pz <= mg * (cam.fy + fabs(bb));
        // a non-finite centre fails the comparisons above; keep such a frame (the statement decides per voxel)
        if (!(fabs(px) + fabs(py) + fabs(pz) < 1e300)) k = true;
        nkept += k;
      }
      keep[t] = k;
    }
    __syncthreads();
    const int fend = min(cam.F - base, TS_THREADS);
    for (int ff = 0; ff < fend; ++ff) {
      if (!keep[ff]) continue;   // the same for every thread of the workgroup
      const int f = base + ff;
      const double *E = ext + (int64_t)f * 12;
      const uint16_t *D = depth + (int64_t)f * cam.H * cam.W;
      const double sx = E[0] * x + E[1] * y, sy = E[4] * x + E[5] * y, sz = E[8] * x + E[9] * y;
#pragma unroll
      for (int k = 0; k < VPT; ++k) {
        const double pz = (sz + E[10] * z[k]) + E[11];
        if (!(pz > 0.0)) continue;
        const double px = (sx + E[2] * z[k]) + E[3];
        const double py = (sy + E[6] * z[k]) + E[7];
        const double uf = ((cam.fx * px) / pz + cam.cx) + 0.5;
        const double vf = ((cam.fy * py) / pz + cam.cy) + 0.5;
        if (!(uf >= 0.0 && uf < Wd && vf >= 0.0 && vf < Hd)) continue;
        const int u = (int)uf, v = (int)vf;
        const double d = dlut[D[v * cam.W + u]];
        if (!(d >= 0.0)) continue;
        const double sdf = (d - pz) * mtab[v * cam.W + u];
        if (!(sdf > -cam.trunc)) continue;
        const double val = fmin(1.0, sdf / cam.trunc);
        const double w = (double)weight[k];
        tsdf[k] = (float)(((double)tsdf[k] * w + val) / (w + 1.0));
        weight[k] += 1;
        if constexpr (COLOR) {
          const uint8_t *c = color + ((int64_t)f * cam.H * cam.W + (v * cam.W + u)) * 3;
#pragma unroll
          for (int e = 0; e < 3; ++e) rgb[k][e] += (int32_t)c[e];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    tsdf_out[(int64_t)b * V + part * PART + t + TS_THREADS * k] = tsdf[k];
    weight_out[(int64_t)b * V + part * PART + t + TS_THREADS * k] = weight[k];
  }
  if constexpr (COLOR) {
    // the slab's sums are PART * 3 consecutive words: voxel t + 256 k of the slab at stage[(t + 256 k) * 3 ..]
#pragma unroll
    for (int k = 0; k < VPT; ++k)
#pragma unroll
      for (int e = 0; e < 3; ++e) stage[(t + TS_THREADS * k) * 3 + e] = rgb[k][e];
    __syncthreads();
    int32_t *out = rgb_out + ((int64_t)b * V + part * PART) * 3;
#pragma unroll
    for (int j = 0; j < VPT * 3; ++j) out[t + TS_THREADS * j] = stage[t + TS_THREADS * j];
  }
  if (kept && nkept && part == 0) atomicAdd(kept, (unsigned long long)nkept);
}

// Zero crossings of one block (of one slab of a 16^3 block: slabs are consecutive ranges of l, so numbering the workgroups
// block-major keeps the output order).  Thread t owns the voxels [t VPT, (t + 1) VPT) of the slab in ascending l -- 8 or 16
// contiguous bytes per lane and array, a coalesced load -- so a workgroup-wide exclusive scan of the threads' counts is a
// voxel's place in the workgroup's output.  WRITE = 0: counts[workgroup] only.  WRITE = 1: the same tests again and the
// points, from base[workgroup] on.  The +x / +y / +z neighbour blocks are looked up once per workgroup.  COLOR (compile
// time, with WRITE = 1; without it the kernel is the depth-only one): the point's colour too, from the ends' colour sums.
template <int B, int WRITE, bool COLOR = false>
__global__ void __launch_bounds__(TS_THREADS)
    ts_extract(const int32_t *__restrict__ bkeys, const float *__restrict__ tsdf, const int32_t *__restrict__ weight,
               const int32_t *__restrict__ table, uint32_t mask, const int32_t *__restrict__ keys, const int32_t *__restrict__ rank,
               double voxel, int min_weight, int32_t *__restrict__ counts, const int32_t *__restrict__ base, int64_t max_points,
               double *__restrict__ xyz, const int32_t *__restrict__ rgb, double *__restrict__ pcolor) {
#pragma clang fp contract(off)
  constexpr int SPLIT = TsdfSplit<B>::value, PART = B * B * B / SPLIT;
  constexpr int V = B * B * B, VPT = PART / TS_THREADS;
  __shared__ int32_t nbr[3];
  __shared__ int32_t lds[TS_THREADS / 64];
  const int b = blockIdx.x / SPLIT, part = blockIdx.x % SPLIT, t = threadIdx.x;
  const int32_t bc[3] = {bkeys[(int64_t)b * 3], bkeys[(int64_t)b * 3 + 1], bkeys[(int64_t)b * 3 + 2]};
  if (t < 3) {
    int32_t q[3] = {bc[0], bc[1], bc[2]};
    q[t] += 1;
    const int row = dgr_lookup<3>(table, mask, keys, q);
    nbr[t] = row < 0 ? -1 : rank[row];
  }
  __syncthreads();
  const float *T0 = tsdf + (int64_t)b * V;
  const int32_t *W0 = weight + (int64_t)b * V;
  constexpr int STR[3] = {1, B, B * B};
  auto crossing = [&](int l, const int lc[3], int a, float f0, float &f1) -> bool {
    int32_t w1;
    if (lc[a] + 1 < B) {
      f1 = T0[l + STR[a]];
      w1 = W0[l + STR[a]];
    } else {
      const int nbk = nbr[a];
      if (nbk < 0) return false;
      const int64_t o = (int64_t)nbk * V + (l - (B - 1) * STR[a]);
      f1 = tsdf[o];
      w1 = weight[o];
    }
    return tsdf_usable(f1, w1, min_weight) && ((f0 < 0.f) != (f1 < 0.f));
  };
  int mine = 0;
  for (int k = 0; k < VPT; ++k) {
    const int l = part * PART + t * VPT + k;
    const float f0 = T0[l];
    if (!tsdf_usable(f0, W0[l], min_weight)) continue;
    const int lc[3] = {l % B, (l / B) % B, l / (B * B)};
    for (int a = 0; a < 3; ++a) {
      float f1;
      mine += crossing(l, lc, a, f0, f1);
    }
  }
  int32_t total;
  const int32_t before = dgr_block_exclusive<int32_t, TS_THREADS>(mine, lds, &total);
  if (!WRITE) {
    if (t == 0) counts[blockIdx.x] = total;
    return;
  }
  int64_t at = (int64_t)base[blockIdx.x] + before;
  for (int k = 0; k < VPT; ++k) {
    const int l = part * PART + t * VPT + k;
    const float f0 = T0[l];
    if (!tsdf_usable(f0, W0[l], min_weight)) continue;
    const int lc[3] = {l % B, (l / B) % B, l / (B * B)};
    for (int a = 0; a < 3; ++a) {
      float f1;
      if (!crossing(l, lc, a, f0, f1)) continue;
      if (at < max_points) {   // (always: the host checked P <= max_points before this launch)
        double p[3];
        const double r = tsdf_crossing_point<B>(bc, lc, a, f0, f1, voxel, p);
#pragma unroll
        for (int e = 0; e < 3; ++e) xyz[at * 3 + e] = p[e];
        if constexpr (COLOR) {   // the two ends once more: the voxel and the neighbour `crossing` read
          const int64_t o0 = (int64_t)b * V + l;
          const int64_t o1 = lc[a] + 1 < B ? o0 + STR[a] : (int64_t)nbr[a] * V + (l - (B - 1) * STR[a]);
          double c[3];
          tsdf_crossing_color(rgb + o0 * 3, weight[o0], rgb + o1 * 3, weight[o1], r, c);
#pragma unroll
          for (int e = 0; e < 3; ++e) pcolor[at * 3 + e] = c[e];
        }
      }
      ++at;
    }
  }
}

template <int B>
static int ts_run_blocks(const int32_t *bkeys, int64_t nb, const uint16_t *depth, const double *dlut, const double *mtab,
                         const double *ext, const TsCam &cam, float *tsdf, int32_t *weight, unsigned long long *kept,
                         const int32_t *table, uint32_t mask, const int32_t *keys, const int32_t *rank, int min_weight,
                         int32_t *counts, const uint8_t *color, int32_t *rgb, hipStream_t stream) {
  const unsigned grid = (unsigned)(nb * TsdfSplit<B>::value);
  if (color)
    ts_integrate<B, true><<<grid, TS_THREADS, 0, stream>>>(bkeys, depth, dlut, mtab, ext, cam, tsdf, weight, kept, color, rgb);
  else
    ts_integrate<B, false><<<grid, TS_THREADS, 0, stream>>>(bkeys, depth, dlut, mtab, ext, cam, tsdf, weight, kept, nullptr, nullptr);
  ts_extract<B, 0><<<grid, TS_THREADS, 0, stream>>>(bkeys, tsdf, weight, table, mask, keys, rank, cam.voxel, min_weight, counts,
                                                    nullptr, 0, nullptr, nullptr, nullptr);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

// The one body of dgr_tsdf_fragment (has_color = false: color, rgb_sum_out and point_color_out are not looked at) and
// dgr_tsdf_fragment_rgb.
static int ts_fragment(dgr_ctx *ctx, const uint16_t *depth, int nframes, int height, int width, const double *intrinsic,
                       const double *pose, const double *extrinsic, double voxel_length, double sdf_trunc, double depth_scale,
                       double depth_trunc, int block, int stride, int min_weight, double *xyz_out, int64_t max_points,
                       int32_t *blocks_out, float *tsdf_out, int32_t *weight_out, int64_t max_blocks, int64_t *n_blocks_out,
                       int64_t *n_points_out, int64_t *kept_out, bool has_color, const uint8_t *color, int32_t *rgb_sum_out,
                       double *point_color_out, dgr_stream stream_) {
  // argument errors first: nothing has touched the device when one of them is reported
  DGR_REQUIRE(ctx && depth && intrinsic && pose && extrinsic && n_blocks_out && n_points_out, "dgr_tsdf_fragment: NULL argument");
  DGR_REQUIRE(xyz_out || max_points == 0, "dgr_tsdf_fragment: xyz_out is NULL but max_points = %lld", (long long)max_points);
  const bool want_volume = blocks_out || tsdf_out || weight_out || (has_color && rgb_sum_out);
  DGR_REQUIRE(!want_volume || (blocks_out && tsdf_out && weight_out),
              "dgr_tsdf_fragment: blocks_out, tsdf_out and weight_out go together");
  if (has_color) {
    DGR_REQUIRE(color, "dgr_tsdf_fragment_rgb: color is NULL");
    DGR_REQUIRE(!want_volume || rgb_sum_out, "dgr_tsdf_fragment_rgb: rgb_sum_out goes together with blocks_out, tsdf_out and weight_out");
    DGR_REQUIRE(nframes <= DGR_TSDF_COLOR_MAX_FRAMES, "dgr_tsdf_fragment_rgb: %d frames: more than %d, a voxel's colour sum could pass 2^31",
                nframes, DGR_TSDF_COLOR_MAX_FRAMES);
  }
  DGR_REQUIRE(max_points >= 0 && max_blocks >= 0, "dgr_tsdf_fragment: negative capacity");
  DGR_REQUIRE(nframes >= 1 && height >= 1 && width >= 1, "dgr_tsdf_fragment: depth must be [F,H,W] with F, H, W >= 1, got [%d,%d,%d]",
              nframes, height, width);
  DGR_REQUIRE(block == 8 || block == 16, "dgr_tsdf_fragment: block must be 8 or 16, got %d", block);
  DGR_REQUIRE(stride >= 1, "dgr_tsdf_fragment: stride = %d", stride);
  DGR_REQUIRE(min_weight >= 1, "dgr_tsdf_fragment: min_weight = %d", min_weight);
  DGR_REQUIRE(voxel_length > 0.0 && std::isfinite(voxel_length), "dgr_tsdf_fragment: voxel_length must be positive and finite");
  const double bl = voxel_length * (double)block;
  DGR_REQUIRE(sdf_trunc > 0.0 && sdf_trunc <= bl, "dgr_tsdf_fragment: sdf_trunc must lie in (0, voxel_length * block]");
  DGR_REQUIRE(depth_scale > 0.0 && std::isfinite(depth_scale), "dgr_tsdf_fragment: depth_scale must be positive and finite");
  DGR_REQUIRE(depth_trunc > 0.0 && std::isfinite(depth_trunc), "dgr_tsdf_fragment: depth_trunc must be positive and finite");
  for (int e = 0; e < 4; ++e) DGR_REQUIRE(std::isfinite(intrinsic[e]), "dgr_tsdf_fragment: non-finite intrinsics");
  DGR_REQUIRE(intrinsic[0] > 0.0 && intrinsic[1] > 0.0, "dgr_tsdf_fragment: fx and fy must be positive");
  for (int f = 0; f < nframes; ++f)
    for (int e = 0; e < 12; ++e)
      DGR_REQUIRE(std::isfinite(pose[(size_t)f * 16 + e]) && std::isfinite(extrinsic[(size_t)f * 16 + e]),
                  "dgr_tsdf_fragment: pose %d is not finite", f);
  DGR_REQUIRE((int64_t)height * width < (1ll << 31), "dgr_tsdf_fragment: 2^31 or more pixels in a frame");
  TsCam cam;
  cam.fx = intrinsic[0], cam.fy = intrinsic[1], cam.cx = intrinsic[2], cam.cy = intrinsic[3];
  cam.voxel = voxel_length, cam.trunc = sdf_trunc, cam.bl = bl, cam.depth_trunc = depth_trunc;
  cam.F = nframes, cam.H = height, cam.W = width, cam.stride = stride;
  cam.Hs = (height + stride - 1) / stride, cam.Ws = (width + stride - 1) / stride;
  const int64_t ns = (int64_t)nframes * cam.Hs * cam.Ws, n = ns * 8;
  DGR_REQUIRE(n < (1ll << 31), "dgr_tsdf_fragment: %lld strided pixels: 2^28 or more (raise the stride)", (long long)ns);
  *n_blocks_out = *n_points_out = 0;
  if (kept_out) *kept_out = 0;

  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  // pinned host memory of the context: [0, 64) the counters the two synchronisations read, then the 3x4 poses and
  // extrinsics, uploaded from there (voxelmean.hip says why)
  const size_t mat_bytes = (size_t)nframes * 12 * sizeof(double);
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64 + 2 * mat_bytes, &pin));
  for (int f = 0; f < nframes; ++f) {
    memcpy(pin + 64 + (size_t)f * 96, pose + (size_t)f * 16, 96);
    memcpy(pin + 64 + mat_bytes + (size_t)f * 96, extrinsic + (size_t)f * 16, 96);
  }
  uint32_t mask;
  double *mats, *dlut, *mtab;
  int32_t *keys, *row_first, *flag, *rank, *table, *counters;   // counters[0] = blocks, [1] = points, [2..3] = kept (u64)
  DGR_ALLOC(mats, A, double, (size_t)nframes * 24);
  DGR_ALLOC(dlut, A, double, 65536);
  DGR_ALLOC(mtab, A, double, (int64_t)height * width);
  DGR_ALLOC(keys, A, int32_t, n * 3);
  DGR_ALLOC(row_first, A, int32_t, n);
  DGR_ALLOC(flag, A, int32_t, n);
  DGR_ALLOC(rank, A, int32_t, n);
  DGR_ALLOC(counters, A, int32_t, 4);
  const double *pose_dev = mats, *ext_dev = mats + (size_t)nframes * 12;
  DGR_HIP_CHECK(hipMemcpyAsync(mats, pin + 64, 2 * mat_bytes, hipMemcpyHostToDevice, stream));
  DGR_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), stream));
  ts_depth_lut<<<65536 / TS_THREADS, TS_THREADS, 0, stream>>>(depth_scale, depth_trunc, dlut);
  ts_multiplier<<<(unsigned)dgr_ceil_div((int64_t)height * width, TS_THREADS), TS_THREADS, 0, stream>>>(cam, mtab);
  const unsigned grid = (unsigned)dgr_ceil_div(n, TS_THREADS);
  ts_candidates<<<(unsigned)dgr_ceil_div(ns, TS_THREADS), TS_THREADS, 0, stream>>>(depth, dlut, pose_dev, cam, ns, keys, row_first);
  DGR_LAUNCH_CHECK();
  DGR_CHECK(dgr_unique_rows(A, keys, n, 3, row_first, nullptr, flag, rank, counters, &table, &mask, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(pin, counters, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // synchronisation 1: the number of blocks sizes the volume
  int32_t nb32;
  memcpy(&nb32, pin, sizeof(nb32));
  const int64_t nb = nb32, V = (int64_t)block * block * block;
  *n_blocks_out = nb;
  if (nb == 0) return DGR_OK;   // no valid pixel: an empty fragment, not an error
  if (want_volume && nb > max_blocks) {
    dgr_set_error("dgr_tsdf_fragment: %lld blocks, room for %lld", (long long)nb, (long long)max_blocks);
    return DGR_ENOMEM;
  }
  if (nb * V * 3 >= (1ll << 31)) {
    dgr_set_error("dgr_tsdf_fragment: %lld blocks of %d^3 voxels: 2^31 or more edges", (long long)nb, block);
    return DGR_ENOMEM;
  }
  int32_t *bkeys = blocks_out, *weight = weight_out, *rgb = has_color ? rgb_sum_out : nullptr, *counts, *base;
  float *tsdf = tsdf_out;
  if (!want_volume) {
    DGR_ALLOC(bkeys, A, int32_t, nb * 3);
    DGR_ALLOC(tsdf, A, float, nb * V);
    DGR_ALLOC(weight, A, int32_t, nb * V);
    if (has_color) DGR_ALLOC(rgb, A, int32_t, nb * V * 3);
  }
  const int64_t ngroups = nb * (block == 16 ? TsdfSplit<16>::value : TsdfSplit<8>::value);   // workgroups of the per-block kernels
  DGR_ALLOC(counts, A, int32_t, ngroups);
  DGR_ALLOC(base, A, int32_t, ngroups);
  ts_blocks<<<grid, TS_THREADS, 0, stream>>>(keys, flag, rank, n, nb, bkeys);
  unsigned long long *kept = kept_out ? reinterpret_cast<unsigned long long *>(counters + 2) : nullptr;
  if (block == 8)
    DGR_CHECK(ts_run_blocks<8>(bkeys, nb, depth, dlut, mtab, ext_dev, cam, tsdf, weight, kept, table, mask, keys, rank,
                               min_weight, counts, has_color ? color : nullptr, rgb, stream));
  else
    DGR_CHECK(ts_run_blocks<16>(bkeys, nb, depth, dlut, mtab, ext_dev, cam, tsdf, weight, kept, table, mask, keys, rank,
                                min_weight, counts, has_color ? color : nullptr, rgb, stream));
  DGR_CHECK(dgr_exclusive_scan_i32(A, counts, base, ngroups, counters + 1, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(pin, counters, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // synchronisation 2: the number of points
  int32_t res[4];
  memcpy(res, pin, sizeof(res));
  const int64_t P = res[1];
  *n_points_out = P;
  if (kept_out) {
    unsigned long long k;
    memcpy(&k, res + 2, sizeof(k));
    *kept_out = (int64_t)k;
  }
  if (P > max_points) {
    dgr_set_error("dgr_tsdf_fragment: %lld points, room for %lld", (long long)P, (long long)max_points);
    return DGR_ENOMEM;
  }
  if (P == 0) return DGR_OK;
  double *pcolor = has_color ? point_color_out : nullptr;
#define TS_EXTRACT_ARGS bkeys, tsdf, weight, table, mask, keys, rank, cam.voxel, min_weight, nullptr, base, max_points, xyz_out, rgb, pcolor
  if (block == 8 && !pcolor) ts_extract<8, 1, false><<<(unsigned)(nb * TsdfSplit<8>::value), TS_THREADS, 0, stream>>>(TS_EXTRACT_ARGS);
  if (block == 8 && pcolor) ts_extract<8, 1, true><<<(unsigned)(nb * TsdfSplit<8>::value), TS_THREADS, 0, stream>>>(TS_EXTRACT_ARGS);
  if (block == 16 && !pcolor) ts_extract<16, 1, false><<<(unsigned)(nb * TsdfSplit<16>::value), TS_THREADS, 0, stream>>>(TS_EXTRACT_ARGS);
  if (block == 16 && pcolor) ts_extract<16, 1, true><<<(unsigned)(nb * TsdfSplit<16>::value), TS_THREADS, 0, stream>>>(TS_EXTRACT_ARGS);
#undef TS_EXTRACT_ARGS
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

extern "C" int dgr_tsdf_fragment(dgr_ctx *ctx, const uint16_t *depth, int nframes, int height, int width,
                                 const double *intrinsic, const double *pose, const double *extrinsic, double voxel_length,
                                 double sdf_trunc, double depth_scale, double depth_trunc, int block, int stride,
                                 int min_weight, double *xyz_out, int64_t max_points, int32_t *blocks_out, float *tsdf_out,
                                 int32_t *weight_out, int64_t max_blocks, int64_t *n_blocks_out, int64_t *n_points_out,
                                 int64_t *kept_out, dgr_stream stream) {
  return ts_fragment(ctx, depth, nframes, height, width, intrinsic, pose, extrinsic, voxel_length, sdf_trunc, depth_scale,
                     depth_trunc, block, stride, min_weight, xyz_out, max_points, blocks_out, tsdf_out, weight_out, max_blocks,
                     n_blocks_out, n_points_out, kept_out, false, nullptr, nullptr, nullptr, stream);
}

extern "C" int dgr_tsdf_fragment_rgb(dgr_ctx *ctx, const uint16_t *depth, int nframes, int height, int width,
                                     const double *intrinsic, const double *pose, const double *extrinsic,
                                     double voxel_length, double sdf_trunc, double depth_scale, double depth_trunc, int block,
                                     int stride, int min_weight, double *xyz_out, int64_t max_points, int32_t *blocks_out,
                                     float *tsdf_out, int32_t *weight_out, int64_t max_blocks, int64_t *n_blocks_out,
                                     int64_t *n_points_out, int64_t *kept_out, const uint8_t *color, int32_t *rgb_sum_out,
                                     double *point_color_out, dgr_stream stream) {
  return ts_fragment(ctx, depth, nframes, height, width, intrinsic, pose, extrinsic, voxel_length, sdf_trunc, depth_scale,
                     depth_trunc, block, stride, min_weight, xyz_out, max_points, blocks_out, tsdf_out, weight_out, max_blocks,
                     n_blocks_out, n_points_out, kept_out, true, color, rgb_sum_out, point_color_out, stream);
}
