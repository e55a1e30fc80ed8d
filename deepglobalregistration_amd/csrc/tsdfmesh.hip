// Triangle mesh and vertex normals of a fused TSDF volume (the reference's util/integration.py: volume.extract_triangle_mesh()
// after the 50 frames): block list + tsdf + weight in, the zero crossings of tsdf.hip's ts_extract as vertices -- same
// points, same order, same bits --, one normal per vertex and the triangles that connect them out.  include/dgr_hip.h at
// dgr_tsdf_mesh states the arithmetic in full; tests/tsdf_mesh_ref.py is the same statement in numpy; mc_table.h (generated
// by tools/gen_mc_table.py) holds the triangles of the 256 sign configurations of a cell.
//
// Passes:
//   ms_insert     the block list enters a hash of its 3-int keys (rebuilt here: the call takes a volume from anywhere); a
//                 coordinate outside [-2^26, 2^26) or a key that is already there raises a flag word
//   ms_pass<0>    ONE WORKGROUP PER 8^3 BLOCK, four slabs per 16^3 block (tsdf.hip's split): the 27 blocks around the
//                 workgroup's are looked up once, the slab's (B+1)^2 x (layers+1) corner states (negative / positive /
//                 unusable) are staged in LDS, and both counts -- crossings and triangles -- come from the states alone
//   scans         a workgroup's first vertex and first triangle                      -- the call's ONE host sync: P, T, flag
//   ms_pass<1>    the same tests again: positions, normals, with colour sums the vertex colours (tsdf_common.h's formula:
//                 the fragment's point colours), and every edge's vertex index (-1: none) into edge_vertex
//   ms_pass<2>    the configurations again: the table's triangles, their corners read from edge_vertex
//
// Determinism: a voxel, its three edges and its cell belong to one thread, output positions come from scans, and the only
// atomics are the hash insertion and the flag word, both order-free.  No floating-point atomics.
#include "dgr_internal.h"
#include "hash.h"
#include "scan.h"
#include "tsdf_common.h"

#define DGR_MC_TABLE_QUALIFIER static __device__ const
#include "mc_table.h"

#include <cmath>
#include <cstring>

constexpr int MS_THREADS = 256;
constexpr int MS_FLAG_RANGE = 1, MS_FLAG_TWICE = 2;
constexpr unsigned char MS_POS = 0, MS_NEG = 1, MS_UNUSABLE = 2;

__global__ void __launch_bounds__(MS_THREADS)
    ms_insert(const int32_t *__restrict__ blocks, int64_t nb, int32_t *table, uint32_t mask, int32_t *flag) {
  const int64_t r = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (r >= nb) return;
  const int32_t me[3] = {blocks[r * 3], blocks[r * 3 + 1], blocks[r * 3 + 2]};
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) inside &= me[a] >= -DGR_TSDF_BLOCK_LIMIT && me[a] < DGR_TSDF_BLOCK_LIMIT;
  if (!inside) {
    atomicOr(flag, MS_FLAG_RANGE);
    return;
  }
  uint32_t slot;
  if (dgr_claim<3>(table, mask, blocks, (int)r, &slot) != DGR_EMPTY) atomicOr(flag, MS_FLAG_TWICE);
}

// The volume as one workgroup sees it: local coordinates in [-1, B + 1] per axis, resolved through the 27 blocks around
// the workgroup's own (nbr[13]); -1 = that block is not in the list.
template <int B>
struct MsView {
  const float *tsdf;
  const int32_t *weight;
  const int32_t *nbr;   // shared, [27]
  __device__ __forceinline__ int64_t at(int x, int y, int z) const {
    const int ox = x < 0 ? -1 : (x >= B ? 1 : 0), oy = y < 0 ? -1 : (y >= B ? 1 : 0), oz = z < 0 ? -1 : (z >= B ? 1 : 0);
    const int n = nbr[(oz + 1) * 9 + (oy + 1) * 3 + (ox + 1)];
    if (n < 0) return -1;
    return (int64_t)n * (B * B * B) + (((z - oz * B) * B + (y - oy * B)) * B + (x - ox * B));
  }
  // F(j; i) of the statement: the neighbour's value if it exists and was observed, else the voxel's own
  __device__ __forceinline__ double value_or(int x, int y, int z, int min_weight, float own) const {
    const int64_t o = at(x, y, z);
    if (o < 0 || weight[o] < min_weight) return (double)own;
    return (double)tsdf[o];
  }
};

// MODE 0: vcounts / tcounts[workgroup].  MODE 1: vertices from vbase[workgroup] on.  MODE 2: triangles from tbase[workgroup] on.
// Thread t owns the voxels (= cells) [t VPT, (t + 1) VPT) of the slab in ascending l, as in ts_extract.  COLOR (compile time,
// with MODE 1; without it the kernel is the one without colour): the vertex's colour too, from the ends' colour sums.
template <int B, int MODE, bool COLOR = false>
__global__ void __launch_bounds__(MS_THREADS)
    ms_pass(const int32_t *__restrict__ blocks, const float *__restrict__ tsdf, const int32_t *__restrict__ weight,
            const int32_t *__restrict__ table, uint32_t mask, double voxel, int min_weight, int32_t *__restrict__ vcounts,
            int32_t *__restrict__ tcounts, const int32_t *__restrict__ vbase, const int32_t *__restrict__ tbase,
            int32_t *__restrict__ edge_vertex, int64_t max_vertices, int64_t max_triangles, double *__restrict__ xyz,
            double *__restrict__ normal, int32_t *__restrict__ tri, const int32_t *__restrict__ rgb, double *__restrict__ color) {
#pragma clang fp contract(off)
  constexpr int SPLIT = TsdfSplit<B>::value, V = B * B * B, PART = V / SPLIT, VPT = PART / MS_THREADS;
  constexpr int LAYERS = B / SPLIT, TX = B + 1, TZ = LAYERS + 1, TILE = TX * TX * TZ;
  __shared__ int32_t nbr[27];
  __shared__ unsigned char state[TILE];
  __shared__ int32_t lds[MS_THREADS / 64];
  const int b = blockIdx.x / SPLIT, part = blockIdx.x % SPLIT, t = threadIdx.x, z0 = part * LAYERS;
  const int32_t bc[3] = {blocks[(int64_t)b * 3], blocks[(int64_t)b * 3 + 1], blocks[(int64_t)b * 3 + 2]};
  if (t < 27) {
    const int32_t q[3] = {(int32_t)((uint32_t)bc[0] + (uint32_t)(t % 3 - 1)), (int32_t)((uint32_t)bc[1] + (uint32_t)((t / 3) % 3 - 1)),
                          (int32_t)((uint32_t)bc[2] + (uint32_t)(t / 9 - 1))};   // (unsigned: a coordinate out of range may wrap)
    nbr[t] = t == 13 ? b : dgr_lookup<3>(table, mask, blocks, q);
  }
  __syncthreads();
  const MsView<B> view{tsdf, weight, nbr};
  for (int i = t; i < TILE; i += MS_THREADS) {
    const int64_t o = view.at(i % TX, (i / TX) % TX, z0 + i / (TX * TX));
    unsigned char s = MS_UNUSABLE;
    if (o >= 0) {
      const float f = tsdf[o];
      if (tsdf_usable(f, weight[o], min_weight)) s = f < 0.f ? MS_NEG : MS_POS;
    }
    state[i] = s;
  }
  __syncthreads();
  auto state_at = [&](int x, int y, int z) -> int { return state[((z - z0) * TX + y) * TX + x]; };
  // a crossing on the +a edge of (x, y, z): both ends usable, signs differ (ts_extract's test)
  auto crossing = [&](int x, int y, int z, int a) -> bool {
    const int s0 = state_at(x, y, z), s1 = state_at(x + (a == 0), y + (a == 1), z + (a == 2));
    return s0 != MS_UNUSABLE && s1 != MS_UNUSABLE && s0 != s1;
  };
  // the cell's configuration, -1 unless all eight corners are usable
  auto config = [&](int x, int y, int z) -> int {
    int cfg = 0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int s = state_at(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2));
      ok &= s != MS_UNUSABLE;
      cfg |= (s == MS_NEG) << c;
    }
    return ok ? cfg : -1;
  };
  int nv = 0, nt = 0;
  for (int k = 0; k < VPT; ++k) {
    const int l = part * PART + t * VPT + k, x = l % B, y = (l / B) % B, z = l / (B * B);
    if (MODE != 2)
      for (int a = 0; a < 3; ++a) nv += crossing(x, y, z, a);
    if (MODE != 1) {
      const int cfg = config(x, y, z);
      nt += cfg < 0 ? 0 : dgr_mc_count[cfg];
    }
  }
  // both counts in one scan: at most 3 VPT 256 = 3072 vertices and 5 VPT 256 = 5120 triangles a workgroup
  int32_t total;
  const int32_t before = dgr_block_exclusive<int32_t, MS_THREADS>(nv | nt << 16, lds, &total);
  if (MODE == 0) {
    if (t == 0) {
      vcounts[blockIdx.x] = total & 0xffff;
      tcounts[blockIdx.x] = total >> 16;
    }
    return;
  }
  if (MODE == 1) {
    int64_t at = (int64_t)vbase[blockIdx.x] + (before & 0xffff);
    for (int k = 0; k < VPT; ++k) {
      const int l = part * PART + t * VPT + k;
      const int lc[3] = {l % B, (l / B) % B, l / (B * B)};
      for (int a = 0; a < 3; ++a) {
        const bool hit = crossing(lc[0], lc[1], lc[2], a);
        edge_vertex[((int64_t)b * V + l) * 3 + a] = hit ? (int32_t)at : -1;
        if (!hit) continue;
        if (at < max_vertices) {   // (always: the host checked P <= max_vertices before this launch)
          int hc[3] = {lc[0], lc[1], lc[2]};
          hc[a] += 1;
          const int64_t o0 = (int64_t)b * V + l, o1 = view.at(hc[0], hc[1], hc[2]);
          const float f0 = tsdf[o0], f1 = tsdf[o1];
          double p[3];
          const double r = tsdf_crossing_point<B>(bc, lc, a, f0, f1, voxel, p);
#pragma unroll
          for (int e = 0; e < 3; ++e) xyz[at * 3 + e] = p[e];
          if constexpr (COLOR) {
            double c[3];
            tsdf_crossing_color(rgb + o0 * 3, weight[o0], rgb + o1 * 3, weight[o1], r, c);
#pragma unroll
            for (int e = 0; e < 3; ++e) color[at * 3 + e] = c[e];
          }
          if (normal) {
            double n[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
              const int dx = e == 0, dy = e == 1, dz = e == 2;
              const double g0 = view.value_or(lc[0] + dx, lc[1] + dy, lc[2] + dz, min_weight, f0)
                                - view.value_or(lc[0] - dx, lc[1] - dy, lc[2] - dz, min_weight, f0);
              const double g1 = view.value_or(hc[0] + dx, hc[1] + dy, hc[2] + dz, min_weight, f1)
                                - view.value_or(hc[0] - dx, hc[1] - dy, hc[2] - dz, min_weight, f1);
              n[e] = g0 + r * (g1 - g0);
            }
            const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
            for (int e = 0; e < 3; ++e) normal[at * 3 + e] = len == 0.0 ? 0.0 : n[e] / len;
          }
        }
        ++at;
      }
    }
    return;
  }
  int64_t at = (int64_t)tbase[blockIdx.x] + (before >> 16);
  for (int k = 0; k < VPT; ++k) {
    const int l = part * PART + t * VPT + k, x = l % B, y = (l / B) % B, z = l / (B * B);
    const int cfg = config(x, y, z);
    if (cfg < 0) continue;
    const int n = dgr_mc_count[cfg];
    for (int j = 0; j < n; ++j, ++at) {
      if (at >= max_triangles) continue;   // (never: the host checked T <= max_triangles before this launch)
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int e = dgr_mc_edges[cfg][j * 3 + v], a = e >> 2;
        // the edge's low corner: bit 0 of e & 3 on the lower other axis, bit 1 on the higher one
        const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;
        int c[3] = {x, y, z};
        c[lo] += e & 1;
        c[hi] += (e >> 1) & 1;
        const int64_t o = view.at(c[0], c[1], c[2]);
        tri[at * 3 + v] = o < 0 ? -1 : edge_vertex[o * 3 + a];   // (o >= 0: the cell's corners all exist)
      }
    }
  }
}

template <int B>
static void ms_launch(int mode, int64_t nb, const int32_t *blocks, const float *tsdf, const int32_t *weight, const int32_t *table,
                      uint32_t mask, double voxel, int min_weight, int32_t *vcounts, int32_t *tcounts, const int32_t *vbase,
                      const int32_t *tbase, int32_t *edge_vertex, int64_t max_vertices, int64_t max_triangles, double *xyz,
                      double *normal, int32_t *tri, const int32_t *rgb, double *color, hipStream_t stream) {
  const unsigned grid = (unsigned)(nb * TsdfSplit<B>::value);
#define MS_ARGS blocks, tsdf, weight, table, mask, voxel, min_weight, vcounts, tcounts, vbase, tbase, edge_vertex, max_vertices, \
                max_triangles, xyz, normal, tri, rgb, color
  if (mode == 0) ms_pass<B, 0><<<grid, MS_THREADS, 0, stream>>>(MS_ARGS);
  if (mode == 1 && !color) ms_pass<B, 1, false><<<grid, MS_THREADS, 0, stream>>>(MS_ARGS);
  if (mode == 1 && color) ms_pass<B, 1, true><<<grid, MS_THREADS, 0, stream>>>(MS_ARGS);
  if (mode == 2) ms_pass<B, 2><<<grid, MS_THREADS, 0, stream>>>(MS_ARGS);
#undef MS_ARGS
}

// The one body of dgr_tsdf_mesh (has_color = false: rgb_sum and color_out are not looked at) and dgr_tsdf_mesh_rgb.
static int ms_mesh(dgr_ctx *ctx, const int32_t *blocks, int64_t n_blocks, const float *tsdf, const int32_t *weight, int block,
                   double voxel_length, int min_weight, double *xyz_out, double *normal_out, int64_t max_vertices,
                   int32_t *tri_out, int64_t max_triangles, int64_t *n_vertices_out, int64_t *n_triangles_out, bool has_color,
                   const int32_t *rgb_sum, double *color_out, dgr_stream stream_) {
  // argument errors first: nothing has touched the device when one of them is reported
  DGR_REQUIRE(ctx && n_vertices_out && n_triangles_out, "dgr_tsdf_mesh: NULL argument");
  DGR_REQUIRE(n_blocks >= 0, "dgr_tsdf_mesh: n_blocks = %lld", (long long)n_blocks);
  DGR_REQUIRE(n_blocks == 0 || (blocks && tsdf && weight), "dgr_tsdf_mesh: NULL argument");
  if (has_color) {
    DGR_REQUIRE(n_blocks == 0 || rgb_sum, "dgr_tsdf_mesh_rgb: rgb_sum is NULL");
    DGR_REQUIRE(color_out || max_vertices == 0, "dgr_tsdf_mesh_rgb: color_out is NULL but max_vertices = %lld", (long long)max_vertices);
  } else {
    rgb_sum = nullptr, color_out = nullptr;
  }
  DGR_REQUIRE(max_vertices >= 0 && max_triangles >= 0, "dgr_tsdf_mesh: negative capacity");
  DGR_REQUIRE(xyz_out || max_vertices == 0, "dgr_tsdf_mesh: xyz_out is NULL but max_vertices = %lld", (long long)max_vertices);
  DGR_REQUIRE(tri_out || max_triangles == 0, "dgr_tsdf_mesh: tri_out is NULL but max_triangles = %lld", (long long)max_triangles);
  DGR_REQUIRE(block == 8 || block == 16, "dgr_tsdf_mesh: block must be 8 or 16, got %d", block);
  DGR_REQUIRE(min_weight >= 1, "dgr_tsdf_mesh: min_weight = %d", min_weight);
  DGR_REQUIRE(voxel_length > 0.0 && std::isfinite(voxel_length), "dgr_tsdf_mesh: voxel_length must be positive and finite");
  *n_vertices_out = *n_triangles_out = 0;
  const int64_t nb = n_blocks, V = (int64_t)block * block * block;
  if (nb == 0) return DGR_OK;   // an empty volume: an empty mesh, not an error
  if (nb >= (1ll << 31) || 5 * nb * V >= (1ll << 31)) {   // 5 nb V < 2^31: vertex (3 nb V) and triangle numbers fit an int32
    dgr_set_error("dgr_tsdf_mesh: %lld blocks of %d^3 voxels: 2^31 or more possible triangles", (long long)nb, block);
    return DGR_ENOMEM;
  }
  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DgrArena &A = ctx->arena;
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64, &pin));
  uint32_t mask;
  const int64_t ngroups = nb * (block == 16 ? TsdfSplit<16>::value : TsdfSplit<8>::value);
  int32_t *table, *counters, *vcounts, *tcounts, *vbase, *tbase, *edge_vertex;   // counters: vertices, triangles, flag
  DGR_CHECK(dgr_table_make(A, nb, &table, &mask, stream));
  DGR_ALLOC(counters, A, int32_t, 4);
  DGR_ALLOC(vcounts, A, int32_t, ngroups);
  DGR_ALLOC(tcounts, A, int32_t, ngroups);
  DGR_ALLOC(vbase, A, int32_t, ngroups);
  DGR_ALLOC(tbase, A, int32_t, ngroups);
  DGR_ALLOC(edge_vertex, A, int32_t, nb * V * 3);
  DGR_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), stream));
  ms_insert<<<(unsigned)dgr_ceil_div(nb, MS_THREADS), MS_THREADS, 0, stream>>>(blocks, nb, table, mask, counters + 2);
  auto launch = [&](int mode) {
    if (block == 8)
      ms_launch<8>(mode, nb, blocks, tsdf, weight, table, mask, voxel_length, min_weight, vcounts, tcounts, vbase, tbase,
                   edge_vertex, max_vertices, max_triangles, xyz_out, normal_out, tri_out, rgb_sum, color_out, stream);
    else
      ms_launch<16>(mode, nb, blocks, tsdf, weight, table, mask, voxel_length, min_weight, vcounts, tcounts, vbase, tbase,
                    edge_vertex, max_vertices, max_triangles, xyz_out, normal_out, tri_out, rgb_sum, color_out, stream);
  };
  launch(0);
  DGR_LAUNCH_CHECK();
  DGR_CHECK(dgr_exclusive_scan_i32(A, vcounts, vbase, ngroups, counters, stream));
  DGR_CHECK(dgr_exclusive_scan_i32(A, tcounts, tbase, ngroups, counters + 1, stream));
  DGR_HIP_CHECK(hipMemcpyAsync(pin, counters, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));   // the one synchronisation: vertices, triangles, the flag word
  int32_t res[4];
  memcpy(res, pin, sizeof(res));
  if (res[2] & MS_FLAG_RANGE) {
    dgr_set_error("dgr_tsdf_mesh: a block coordinate outside [-2^26, 2^26)");
    return DGR_EINVAL;
  }
  if (res[2] & MS_FLAG_TWICE) {
    dgr_set_error("dgr_tsdf_mesh: a block occurs twice in the list");
    return DGR_EINVAL;
  }
  const int64_t P = res[0], T = res[1];
  *n_vertices_out = P;
  *n_triangles_out = T;
  if (P > max_vertices || T > max_triangles) {
    dgr_set_error("dgr_tsdf_mesh: %lld vertices and %lld triangles, room for %lld and %lld", (long long)P, (long long)T,
                  (long long)max_vertices, (long long)max_triangles);
    return DGR_ENOMEM;
  }
  if (P == 0) return DGR_OK;   // (no vertex, no triangle)
  launch(1);
  if (T > 0) launch(2);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}

extern "C" int dgr_tsdf_mesh(dgr_ctx *ctx, const int32_t *blocks, int64_t n_blocks, const float *tsdf, const int32_t *weight,
                             int block, double voxel_length, int min_weight, double *xyz_out, double *normal_out,
                             int64_t max_vertices, int32_t *tri_out, int64_t max_triangles, int64_t *n_vertices_out,
                             int64_t *n_triangles_out, dgr_stream stream) {
  return ms_mesh(ctx, blocks, n_blocks, tsdf, weight, block, voxel_length, min_weight, xyz_out, normal_out, max_vertices, tri_out,
                 max_triangles, n_vertices_out, n_triangles_out, false, nullptr, nullptr, stream);
}

extern "C" int dgr_tsdf_mesh_rgb(dgr_ctx *ctx, const int32_t *blocks, int64_t n_blocks, const float *tsdf, const int32_t *weight,
                                 int block, double voxel_length, int min_weight, double *xyz_out, double *normal_out,
                                 int64_t max_vertices, int32_t *tri_out, int64_t max_triangles, int64_t *n_vertices_out,
                                 int64_t *n_triangles_out, const int32_t *rgb_sum, double *color_out, dgr_stream stream) {
  return ms_mesh(ctx, blocks, n_blocks, tsdf, weight, block, voxel_length, min_weight, xyz_out, normal_out, max_vertices, tri_out,
                 max_triangles, n_vertices_out, n_triangles_out, true, rgb_sum, color_out, stream);
}
