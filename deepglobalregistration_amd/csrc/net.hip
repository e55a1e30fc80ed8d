// ResUNetBN2C (3-D FCGF net and 6-D inlier net) on top of the sparse-conv kernel.
// Replaces model.load_model('ResUNetBN2C')(...) + load_state_dict + eval + forward:
// constructor model/resunet.py:428-596, channel tables :662-665, forward :598-649, residual block
// model/residual_block.py:83-134, eval batch norm model/common.py:11-21.
//
// Load time: eval-mode batch norm is folded into the kernels (scale) and a per-channel shift; the
// kernels are re-tiled on the device into the MFMA B-operand order documented in conv.hip.
// Forward: a loop over the layer table; every conv is one of the kernel families of conv.hip / conv_identity.hip /
// conv1.hip / conv_os.hip / conv_wide.hip (chosen per layer in layer_kind); rule-major layers write per-pair product rows that a deterministic reduction sums on top of the folded
// shift (+ residual).  ReLU is never a separate pass: a tensor carries a "ReLU pending" flag and the consumer applies
// max(x,0) while gathering (or the producer bakes it into the split rows it writes for a wide-layer consumer).
// ME.cat is free: producers write into column ranges of a pre-concatenated buffer (row stride = total channels).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "dgr_internal.h"

constexpr int CH[5] = {0, 32, 64, 128, 256};     // model/resunet.py:664
constexpr int TR[5] = {0, 64, 64, 64, 128};      // model/resunet.py:665
static constexpr float BN_EPS = 1e-5f;

// ---- the forward as data (model/resunet.py:598-649; tests/layer_trace_ref.py holds the same two tables)
// Tensors: level = log2 of the tensor stride; `buf` = the row that owns the buffer (its own index, or the concatenation
// this tensor is the columns [col0, col0 + cols) of: ME.cat is free, producers write into column ranges of a
// pre-concatenated buffer); the row stride is the owner's width; relu = consumers apply max(x, 0) when reading.
// Owners are allocated in table order, and stand in front of the rows that alias them.
enum Tn : int { NO = -1, X, T1, Y1, CAT1, S1T, S1, T2, Y2, CAT2, S2T, S2, T4, Y4, CAT4, S4T, S4, T8, Y8, S8,
                U4, V4, U2, V2, U1, V1, H, OUT, N_TENSORS };
constexpr int W_CIN = -1, W_COUT = -2;   // widths the caller chooses (dgr_net::cin / cout)
struct TensorRow { const char *name; int lvl; Tn buf; int col0, cols, relu; };
static const TensorRow TENSORS[N_TENSORS] = {
    {"X", 0, X, 0, W_CIN, 0},   // the caller's features
    {"T1", 0, T1, 0, CH[1], 0}, {"Y1", 0, Y1, 0, CH[1], 1},
    {"CAT1", 0, CAT1, 0, TR[2] + CH[1], 1}, {"S1T", 0, CAT1, 0, TR[2], 1}, {"S1", 0, CAT1, TR[2], CH[1], 1},
    {"T2", 1, T2, 0, CH[2], 0}, {"Y2", 1, Y2, 0, CH[2], 1},
    {"CAT2", 1, CAT2, 0, TR[3] + CH[2], 1}, {"S2T", 1, CAT2, 0, TR[3], 1}, {"S2", 1, CAT2, TR[3], CH[2], 1},
    {"T4", 2, T4, 0, CH[3], 0}, {"Y4", 2, Y4, 0, CH[3], 1},
    {"CAT4", 2, CAT4, 0, TR[4] + CH[3], 1}, {"S4T", 2, CAT4, 0, TR[4], 1}, {"S4", 2, CAT4, TR[4], CH[3], 1},
    {"T8", 3, T8, 0, CH[4], 0}, {"Y8", 3, Y8, 0, CH[4], 1}, {"S8", 3, S8, 0, CH[4], 1},
    {"U4", 2, U4, 0, TR[4], 0}, {"V4", 2, V4, 0, TR[4], 1},
    {"U2", 1, U2, 0, TR[3], 0}, {"V2", 1, V2, 0, TR[3], 1},
    {"U1", 0, U1, 0, TR[2], 0}, {"V1", 0, V1, 0, TR[2], 1},
    {"H", 0, H, 0, TR[1], 1},
    {"OUT", 0, OUT, 0, W_COUT, 0}};   // the caller's output (a buffer of the forward's while it is not normalised yet)
// ... and the block outputs that dgr_net_get_intermediate serves (as f32 rows, ReLU applied), by their names in the model
static const struct { const char *name; Tn t; } INTERMEDIATES[] = {
    {"s1", S1}, {"s2", S2}, {"s4", S4}, {"s8", S8}, {"s4_tr", S4T}, {"s2_tr", S2T}, {"s1_tr", S1T}};

// Layers in forward order.  The map says which kernel map and which kernel volume: conv1's ks^D at stride 1; the 3^D
// map of the tensors' level (same), into the next coarser level (down), or that one with in / out swapped (up: the
// transposed convs); none (identity, kernel volume 1).  A layer's Cin / Cout are its tensors' widths.
enum Map : int { M_CONV1, M_SAME, M_DOWN, M_UP, M_IDENT };
struct LayerRow { const char *name, *norm; bool bias; Map map; Tn in, out, res; };
#define DGR_BLOCK(b, a, y, s) {b ".conv1", b ".norm1", false, M_SAME, a, y, NO}, {b ".conv2", b ".norm2", false, M_SAME, y, s, a}
static const LayerRow LAYERS[] = {
    {"conv1", "norm1", false, M_CONV1, X, T1, NO},             DGR_BLOCK("block1", T1, Y1, S1),
    {"conv2", "norm2", false, M_DOWN, S1, T2, NO},             DGR_BLOCK("block2", T2, Y2, S2),
    {"conv3", "norm3", false, M_DOWN, S2, T4, NO},             DGR_BLOCK("block3", T4, Y4, S4),
    {"conv4", "norm4", false, M_DOWN, S4, T8, NO},             DGR_BLOCK("block4", T8, Y8, S8),
    {"conv4_tr", "norm4_tr", false, M_UP, S8, U4, NO},         DGR_BLOCK("block4_tr", U4, V4, S4T),
    {"conv3_tr", "norm3_tr", false, M_UP, CAT4, U2, NO},       DGR_BLOCK("block3_tr", U2, V2, S2T),
    {"conv2_tr", "norm2_tr", false, M_UP, CAT2, U1, NO},       DGR_BLOCK("block2_tr", U1, V1, S1T),
    {"conv1_tr", nullptr, false, M_IDENT, CAT1, H, NO},        // no bias, no BN: residual_block.py:38-44
    {"final", nullptr, true, M_IDENT, H, OUT, NO}};            // the only bias: resunet.py:589-596
#undef DGR_BLOCK
constexpr int N_LAYERS = sizeof(LAYERS) / sizeof(LAYERS[0]);
static_assert(N_LAYERS == 23, "ResUNetBN2C has 23 convs");

// Which kernel runs a layer (layer_kind, the one place that decides it)
enum Kind : int {
  K_NONE,         // no forward yet
  K_CONV1_FUSED,  // conv1 fused with its neighbour search (dgr_conv1_probe, conv1.hip)
  K_SMALL_CIN,    // conv1 with Cin <= 8, output-stationary over the rule-major map (conv1.hip)
  K_RULE,         // rule-major f32 product rows + reduction (conv.hip)
  K_WIDE,         // rule-major product rows from split rows, f16x2 (conv_wide.hip) + reduction
  K_OS_F32,       // output-stationary over neighbour tables, list-based, f32 operands (conv_os.hip)
  K_OS,           // the same with split operands
  K_DENSE,        // dense tiles (conv_dense.hip)
  K_UP,           // transposed conv by parity class (conv_up.hip)
  K_IDENTITY};    // kernel volume 1 (conv_identity.hip)
static bool on_tables(Kind k) { return k == K_OS_F32 || k == K_OS || k == K_DENSE || k == K_UP; }
static bool reads_amax(Kind k) { return k == K_OS || k == K_DENSE || k == K_UP; }
static bool writes_amax(Kind k) { return k == K_CONV1_FUSED || on_tables(k); }   // (their epilogues can)
static bool rule_major(Kind k) { return k == K_RULE || k == K_WIDE; }   // product rows + the reduction: it alone can write split rows

struct DgrLayer {
  std::string name;
  int K, cin, cout, cin_pad, cout_pad;
  // device operand layouts: views into DgrWeights::allocs (which owns them)
  float *w = nullptr;      // tiled
  float *w16 = nullptr;    // 16x16x4 fragment order (3-D K = 27 layers: output-stationary conv, conv_os.hip)
  void *w16b = nullptr;    // the same as two f16 pieces in 16x16x32 fragment order (conv_os.hip)
  void *w16d = nullptr;    // the pieces once more in the channel order of the dense-tile kernel's gather (conv_dense.hip)
  int64_t w16b_piece = 0;
  float *wc = nullptr;     // conv1 weights in the operand order of conv1_grid_mfma (3-D conv1 with one input channel)
  float *wq = nullptr;     // conv1 weights quad-major for conv_cin6_quad_kernel (6-D conv1 with six input channels)
  void *wb = nullptr;      // two f16 pieces in 32x32x16 fragment order (wide layers, conv_wide.hip)
  int64_t wb_piece = 0;    // 16-byte units per piece
  float w_unscale = 1.f;   // wb / w16b hold the two f16 pieces of 2^e W; w_unscale = 2^-e
  float *shift = nullptr;  // [cout] or nullptr
};

// One layer of the last forward as it was launched: what dgr_net_rerun_layer replays and dgr_net_layer_stats counts
struct LayerRun {
  Kind kind = K_NONE;
  const int32_t *n_in = nullptr, *n_out = nullptr;
  int64_t n_out_cap = 0;
  int K = 1;
  DgrConvLaunch launch;   // phase 1 of K_RULE / K_WIDE / K_IDENTITY; the tensors of K_SMALL_CIN and K_CONV1_FUSED
  DgrSplitRows split_in;  // K_WIDE: the input as split rows
  DgrKernelMap km;        // K_SMALL_CIN: its map (copies: the map set itself lives on the forward's stack)
  DgrConvOsLaunch os;     // the kinds on neighbour tables ...
  DgrNbrTable nbr;        // ... and their table (os.nbr points here)
  DgrCoordMap cm0;        // K_CONV1_FUSED: the coordinate map it searches, its device pair counter, the row maxima it leaves
  int32_t *fused_pairs = nullptr;
  uint32_t *fused_amax = nullptr;
  const int32_t *rule_ptr = nullptr;   // the kinds on pair lists: pairs per offset (dgr_net_layer_stats)
  // phase 2 of K_RULE / K_WIDE: the reduction
  const int32_t *red_ptr = nullptr, *red_pos = nullptr;
  const float *res = nullptr;
  int res_ld = 0, res_relu = 0, out_relu = 0;
  DgrSplitRows split_out;   // what the reduction also writes
  bool split_only = false;  // ... and the only thing
};

// One tensor of a forward in every form it has
struct Tensor {
  float *ptr = nullptr;
  int ld = 0;
  int relu = 0;  // consumers must apply ReLU when reading
  DgrSplitRows split;   // set for tensors a wide layer gathers: written by the tensor's producer (ReLU applied)
  bool split_only = false;   // ... and nobody reads the f32 rows (a block's middle tensor): they are not written
  // 3-D net: per row the bits of its largest |x| (after the pending ReLU), left behind by the tensor's producer for the
  // split-operand consumers (conv_os.hip / conv_dense.hip); amax2: the same array of the concatenation this tensor is a
  // column range of.  Zero-initialised, filled by atomicMax.
  uint32_t *amax = nullptr, *amax2 = nullptr;
  // 3-D net: the rows as ready-made operand pieces of the dense-tile kernel (conv_dense.hip, "dense split rows": 4 x
  // channels bytes per row), written by the tensor's producer; dsplit_only: nobody reads the f32 rows (a block's middle
  // tensor) -- they are not written and `dsplit` is the tensor's own buffer
  unsigned char *dsplit = nullptr;
  bool dsplit_only = false;
  // 3-D net, tensors between the output-stationary kernels and the wide rule-major layers of the coarse levels: the
  // producer could not leave the representation the consumer reads, so the consumer's launch makes it first --
  // split_pending: `split` from the f32 rows (dgr_split_rows); amax_pending: `amax` from the f32 rows (dgr_row_amax)
  bool split_pending = false, amax_pending = false;
};

// The immutable half of a net: the folded, re-tiled weights in HBM.  Shared (reference-counted) by every dgr_net made
// from it with dgr_net_share -- one context per HIP stream, ONE weight set per device.
struct DgrWeights {
  std::vector<DgrLayer> layers;  // 23 convs in forward order
  std::vector<void *> allocs;    // every device buffer the layers point into, recorded as soon as it is allocated
  int64_t param_bytes = 0;
  int device = 0;
  template <class T> int alloc(T **p, size_t n) {
    DGR_HIP_CHECK(hipMalloc((void **)p, n * sizeof(T)));
    allocs.push_back(*p);
    DGR_CHECK(dgr_fill_fresh(*p, n * sizeof(T)));
    return DGR_OK;
  }
  // Runs on whichever host thread drops the last reference (e.g. Python's GC inside a worker thread): the thread's current
  // device is restored afterwards; the synchronisation stalls every stream of THIS device once, when the last sharer goes.
  ~DgrWeights() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (void *p : allocs) (void)hipFree(p);
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  }
};

// ... and the per-context half: what the last forward of THIS net object left behind
struct dgr_net {
  dgr_ctx *ctx;
  int D, cin, cout, conv1_ks, normalize;
  std::shared_ptr<DgrWeights> W;
  LayerRun runs[N_LAYERS];
  Tensor tensors[N_TENSORS];     // by Tn: every tensor in the forms the last forward really wrote (dgr_net_get_tensor)
  DgrCoordMap levels[4];         // ... and their coordinate maps (row counts, row numbering)
  uint64_t run_generation = 0;   // arena generation `runs` / `tensors` point into
  int width(Tn t) const { return TENSORS[t].cols == W_CIN ? cin : TENSORS[t].cols == W_COUT ? cout : TENSORS[t].cols; }
  // 3-D net on neighbour tables: the 128 / 256-channel layers of the two coarse levels run on the wide rule-major kernel
  // (dgr_net_set_wide_coarse; off: every K = 27 layer output-stationary, with row maxima behind every tensor)
  bool wide_coarse = false;
};

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

static const dgr_weight_desc *find_desc(const dgr_weight_desc *w, int n, const std::string &name) {
  for (int i = 0; i < n; ++i)
    if (name == w[i].name) return &w[i];
  return nullptr;
}

// ---- weight preparation: HIP kernels turn the [K, cin, cout] kernel tensor in HBM (the caller's with
// dgr_net_create_device, uploaded by dgr_net_create) into every operand layout the conv kernels read, one elementwise
// kernel per layout; only the per-channel batch-norm vectors (cout floats each) are folded on the host.
template <class F>
__global__ void __launch_bounds__(256) dgr_fill_kernel(int64_t n, F f) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) f(o);
}
template <class F>
static int dgr_fill(hipStream_t s, int64_t n, F f) {
  if (n <= 0) return DGR_OK;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 1 << 16);
  dgr_fill_kernel<<<(int)blocks, 256, 0, s>>>(n, f);
  DGR_LAUNCH_CHECK();
  return DGR_OK;
}
__device__ __forceinline__ uint16_t dgr_f16_bits_dev(float x) {
  const _Float16 h = (_Float16)x;
  return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float dgr_f16_val_dev(float x) { return (float)(_Float16)x; }
__global__ void __launch_bounds__(256) dgr_absmax_scaled_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                                                int64_t n, int cout, uint32_t *out_bits) {
  float mx = 0.f;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256)
    mx = fmaxf(mx, fabsf(__fmul_rn(w[o], scale[o % cout])));
  for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out_bits, __float_as_uint(mx));   // non-negative floats order like their bits
}

// One net_create's preparation state: a private stream (default flags: ordered after the caller's NULL-stream work) and
// device temporaries that every layer reuses in stream order; released on every exit.
struct WeightPrep {
  bool dev;                    // the descriptors hold device pointers (dgr_net_create_device)
  hipStream_t s = nullptr;
  float *sc = nullptr;         // the layer's scale[] (cout <= 256)
  uint32_t *mxb = nullptr;     // the layer's largest |w| (bits)
  float *staging = nullptr;    // dgr_net_create: the layer's kernel tensor, uploaded (staging_n floats)
  size_t staging_n = 0;
  ~WeightPrep() {
    if (s) (void)hipStreamSynchronize(s);
    (void)hipFree(sc); (void)hipFree(mxb); (void)hipFree(staging);
    if (s) (void)hipStreamDestroy(s);
  }
};

static int make_layer(dgr_net *net, WeightPrep &P, const dgr_weight_desc *descs, int nd, const LayerRow &row, int K) {
  const std::string name = row.name;
  const char *bn = row.norm;
  const bool bias = row.bias;
  const int cin = net->width(row.in), cout = net->width(row.out);
  DgrLayer L;
  L.name = name;
  L.K = K; L.cin = cin; L.cout = cout;
  L.cin_pad = round_up(cin, 8);
  L.cout_pad = cout <= 32 ? 32 : cout <= 64 ? 64 : cout <= 128 ? 128 : 256;
  // conv1 is the one layer whose Cin the caller chooses: zero-pad to the next width the rule-major kernel is built for
  if (L.cout_pad == 32 && L.cin_pad > 8) {
    DGR_REQUIRE(cin <= 64, "%s: %d input channels (at most 64 into a 32-channel layer)", name.c_str(), cin);
    L.cin_pad = cin <= 32 ? 32 : 64;
  }
  DGR_REQUIRE(cout <= 256 && cin <= 256, "%s: channel count above 256 not supported", name.c_str());
  const dgr_weight_desc *kd = find_desc(descs, nd, name + ".kernel");
  DGR_REQUIRE(kd != nullptr, "state_dict is missing '%s.kernel'", name.c_str());
  // kernel-volume-1 convs are stored [Cin,Cout] by ME 0.5.x and [1,Cin,Cout] by 0.4-era checkpoints
  DGR_REQUIRE(kd->numel == (int64_t)K * cin * cout, "'%s.kernel' has %lld elements, expected %d x %d x %d",
              name.c_str(), (long long)kd->numel, K, cin, cout);
  std::vector<float> scale(cout, 1.f), shift(cout, 0.f);
  bool has_shift = false;
  // the per-channel tensors (batch norm, bias: cout floats each) are folded on the host either way; `dev`: fetched first
  std::vector<std::vector<float>> small;
  auto host_of = [&](const dgr_weight_desc *d) -> const float * {
    if (!P.dev) return d->data;
    small.emplace_back((size_t)d->numel);
    if (hipMemcpy(small.back().data(), d->data, (size_t)d->numel * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
    return small.back().data();
  };
  if (bn) {
    std::string p = std::string(bn) + ".bn.";
    const dgr_weight_desc *g = find_desc(descs, nd, p + "weight"), *b = find_desc(descs, nd, p + "bias"),
                          *m = find_desc(descs, nd, p + "running_mean"),
                          *v = find_desc(descs, nd, p + "running_var");
    DGR_REQUIRE(g && b && m && v, "state_dict is missing batch-norm tensors '%s*'", p.c_str());
    DGR_REQUIRE(g->numel == cout && b->numel == cout && m->numel == cout && v->numel == cout,
                "batch-norm '%s' has the wrong width", p.c_str());
    const float *gd = host_of(g), *bd2 = host_of(b), *md = host_of(m), *vd = host_of(v);
    DGR_REQUIRE(gd && bd2 && md && vd, "batch-norm '%s': device tensors could not be read", p.c_str());
    for (int c = 0; c < cout; ++c) {
      float s = gd[c] / sqrtf(vd[c] + BN_EPS);
      scale[c] = s;
      shift[c] = bd2[c] - md[c] * s;
    }
    has_shift = true;
  }
  if (bias) {
    const dgr_weight_desc *bd = find_desc(descs, nd, name + ".bias");
    DGR_REQUIRE(bd && bd->numel == cout, "state_dict is missing '%s.bias' [1,%d]", name.c_str(), cout);
    const float *bh = host_of(bd);
    DGR_REQUIRE(bh, "'%s.bias': device tensor could not be read", name.c_str());
    for (int c = 0; c < cout; ++c) shift[c] += bh[c];
    has_shift = true;
  }
  DgrWeights &W = *net->W;
  hipStream_t s = P.s;
  const float *src = kd->data;   // [K, cin, cout] f32 on the device
  if (!P.dev) {
    const size_t n = (size_t)kd->numel;
    if (n > P.staging_n) {   // grown once the earlier layers' fills are done with it
      DGR_HIP_CHECK(hipStreamSynchronize(s));
      DGR_HIP_CHECK(hipFree(P.staging));
      P.staging = nullptr;
      DGR_HIP_CHECK(hipMalloc((void **)&P.staging, n * sizeof(float)));
      DGR_CHECK(dgr_fill_fresh(P.staging, n * sizeof(float)));
      P.staging_n = n;
    }
    DGR_HIP_CHECK(hipMemcpyAsync(P.staging, kd->data, n * sizeof(float), hipMemcpyHostToDevice, s));
    src = P.staging;
  }
  const float *sc = P.sc;
  DGR_HIP_CHECK(hipMemcpyAsync(P.sc, scale.data(), (size_t)cout * sizeof(float), hipMemcpyHostToDevice, s));
  if (has_shift) {
    DGR_CHECK(W.alloc(&L.shift, cout));
    DGR_HIP_CHECK(hipMemcpyAsync(L.shift, shift.data(), (size_t)cout * sizeof(float), hipMemcpyHostToDevice, s));
  }
  // the layer's weight scale: the largest |w| (batch norm folded in) lands in [2^14, 2^15)
  const int64_t nw = (int64_t)K * cin * cout;
  DGR_HIP_CHECK(hipMemsetAsync(P.mxb, 0, sizeof(uint32_t), s));
  dgr_absmax_scaled_kernel<<<(int)std::min<int64_t>((nw + 255) / 256, 4096), 256, 0, s>>>(src, sc, nw, cout, P.mxb);
  DGR_LAUNCH_CHECK();
  uint32_t bits = 0;
  DGR_HIP_CHECK(hipMemcpyAsync(&bits, P.mxb, sizeof(bits), hipMemcpyDeviceToHost, s));
  DGR_HIP_CHECK(hipStreamSynchronize(s));   // w_scale is a kernel argument below (and the host vectors are consumed)
  float mx;
  memcpy(&mx, &bits, 4);
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) (void)frexpf(mx, &ex);   // mx in [2^(ex-1), 2^ex)
  ex = std::min(std::max(ex, -100), 100);
  const float w_scale = ldexpf(1.f, 15 - ex);
  L.w_unscale = ldexpf(1.f, ex - 15);
  const bool use_wide = K > 1 && !dgr_exact_f32() && dgr_conv_wide_supported(L.cin_pad, cin, cout) && !(net->D == 3 && K == 27);
  // 3-D nets that run on neighbour tables: the same-stride and strided (not the transposed) 128 / 256-channel layers of
  // the two coarse levels ALSO get the wide kernel's operands -- they run on it over lists derived from the tables
  // (layer_kind), next to the w16 / w16b copies of the output-stationary kernel, which DGR_NO_WIDE3=1 still selects
  const bool transposed = row.map == M_UP;
  const bool wide3 = net->D == 3 && K == 27 && net->cin <= 8 && net->conv1_ks <= 7 && !transposed && !dgr_exact_f32() &&
                     cin >= 128 && cout >= 128 && dgr_conv_wide_supported(L.cin_pad, cin, cout);
  if (use_wide || wide3) {
    const int S16 = cin / 16, NB32 = cout / 32;
    L.wb_piece = (int64_t)K * S16 * NB32 * 64;
    const int64_t ne = L.wb_piece * 8;
    uint16_t *dst;
    DGR_CHECK(W.alloc(&dst, (size_t)2 * ne));
    L.wb = dst;
    DGR_CHECK(dgr_fill(s, ne, [=] __device__(int64_t o) {
      const int e = (int)(o & 7), lane = (int)((o >> 3) & 63);
      const int64_t r = o >> 9;
      const int nb = (int)(r % NB32), s2 = (int)((r / NB32) % S16), k = (int)(r / ((int64_t)NB32 * S16));
      const int col = 32 * nb + (lane & 31), row = 16 * s2 + 8 * (lane >> 5) + e;
      const float xs = __fmul_rn(__fmul_rn(src[((size_t)k * cin + row) * cout + col], sc[col]), w_scale);
      dst[o] = dgr_f16_bits_dev(xs);
      dst[ne + o] = dgr_f16_bits_dev(xs - dgr_f16_val_dev(xs));
    }));
    W.param_bytes += (size_t)2 * ne * sizeof(uint16_t);
  }
  if (!use_wide) {
    const int S = L.cin_pad / 8, NBLK = L.cout_pad / 32;
    const int64_t ne = (int64_t)K * S * NBLK * 256;
    DGR_CHECK(W.alloc(&L.w, ne));
    float *const dst = L.w;
    DGR_CHECK(dgr_fill(s, ne, [=] __device__(int64_t o) {
      const int c = (int)(o & 3), lane = (int)((o >> 2) & 63);
      const int64_t r = o >> 8;
      const int nb = (int)(r % NBLK), s2 = (int)((r / NBLK) % S), k = (int)(r / ((int64_t)NBLK * S));
      const int row = 8 * s2 + 4 * (lane >> 5) + c, col = 32 * nb + (lane & 31);
      dst[o] = (row < cin && col < cout) ? __fmul_rn(src[((size_t)k * cin + row) * cout + col], sc[col]) : 0.f;
    }));
    W.param_bytes += (size_t)ne * sizeof(float);
  }
  if (net->D == 3 && K == 27 && L.cin_pad % 16 == 0 && cout % 32 == 0) {
    // second copy in v_mfma_f32_16x16x4_f32 operand order (conv_os.hip): W16[k][g][jb][lane][c]
    const int GT = L.cin_pad / 16, NB = cout / 16;
    {
      const int64_t ne = (int64_t)K * GT * NB * 256;
      DGR_CHECK(W.alloc(&L.w16, ne));
      float *const dst = L.w16;
      DGR_CHECK(dgr_fill(s, ne, [=] __device__(int64_t o) {
        const int c = (int)(o & 3), lane = (int)((o >> 2) & 63);
        const int64_t r = o >> 8;
        const int jb = (int)(r % NB), g = (int)((r / NB) % GT), k = (int)(r / ((int64_t)NB * GT));
        const int col = 16 * jb + (lane & 15), row = 16 * g + 4 * (lane >> 4) + c;
        dst[o] = row < cin ? __fmul_rn(src[((size_t)k * cin + row) * cout + col], sc[col]) : 0.f;
      }));
      W.param_bytes += (size_t)ne * sizeof(float);
    }
    if (cin % 32 == 0) {
      // WB[piece][k][s][jb][lane] = 8 f16 = piece of W[k][32 s + 8 (lane >> 4) + e][16 jb + (lane & 15)]
      const int S32 = cin / 32;
      L.w16b_piece = (int64_t)K * S32 * NB * 64;
      const int64_t ne = L.w16b_piece * 8;
      uint16_t *pcs;
      DGR_CHECK(W.alloc(&pcs, (size_t)2 * ne));
      L.w16b = pcs;
      DGR_CHECK(dgr_fill(s, ne, [=] __device__(int64_t o) {
        const int e = (int)(o & 7), lane = (int)((o >> 3) & 63);
        const int64_t r = o >> 9;
        const int jb = (int)(r % NB), sI = (int)((r / NB) % S32), k = (int)(r / ((int64_t)NB * S32));
        const int col = 16 * jb + (lane & 15), row = 32 * sI + 8 * (lane >> 4) + e;
        const float xs = __fmul_rn(__fmul_rn(src[((size_t)k * cin + row) * cout + col], sc[col]), w_scale);
        pcs[o] = dgr_f16_bits_dev(xs);
        pcs[ne + o] = dgr_f16_bits_dev(xs - dgr_f16_val_dev(xs));
      }));
      W.param_bytes += (size_t)2 * ne * sizeof(uint16_t);
      if (net->D == 3 && K == 27 && (dgr_conv_dense_supported(cin, L.cin_pad, cout) || dgr_conv_up_supported(cin, L.cin_pad, cout))) {
        // conv_dense.hip (and conv_up.hip, which gathers the same way) reads its weight operands straight from memory: the
        // quad-coalesced gather hands lane (col, lq) the channels 4 lq .. + 3 and 16 + 4 lq .. + 3 of a 32-channel step,
        // so its 16-byte operand is half (lq & 1) of the natural fragments of lanes (col, lq >> 1) and (col, (lq >> 1) + 2)
        uint16_t *pd;
        DGR_CHECK(W.alloc(&pd, (size_t)2 * ne));
        L.w16d = pd;
        DGR_CHECK(dgr_fill(s, 2 * ne, [=] __device__(int64_t o) {   // (fragments of both pieces alike)
          const int e = (int)(o & 3), h = (int)((o >> 2) & 1);
          const int64_t f = o >> 3, base = f & ~(int64_t)63;
          const int lane = (int)(f & 63), col = lane & 15, lq = lane >> 4;
          const int64_t srcf = base + col + 16 * ((lq >> 1) + 2 * h);
          pd[o] = pcs[srcf * 8 + 4 * (lq & 1) + e];
        }));
        W.param_bytes += (size_t)2 * ne * sizeof(uint16_t);
      }
    }
  }
  if (net->D == 3 && name == "conv1" && cin == 1 && cout == 32 && K <= 343) {
    // conv1_grid_mfma (conv1.hip): per z-slab kz and 4-offset step s the A operands of the two v_mfma_f32_16x16x4_f32,
    // wt[kz][s][lane] = {W[k][lane & 15], W[k][16 + (lane & 15)]}, k = kz ks^2 + 4 s + (lane >> 4); zero past the slab
    int ks = 1;
    while (ks * ks * ks < K) ++ks;
    const int ks2 = ks * ks, steps = (ks2 + 3) / 4;
    const int64_t ne = (int64_t)ks * steps * 128;
    DGR_CHECK(W.alloc(&L.wc, ne));
    float *const dst = L.wc;
    DGR_CHECK(dgr_fill(s, ne, [=] __device__(int64_t o) {
      const int j = (int)(o & 1), lane = (int)((o >> 1) & 63);
      const int64_t r = o >> 7;
      const int s2 = (int)(r % steps), kz = (int)(r / steps);
      const int kk = 4 * s2 + (lane >> 4), col = (lane & 15) + 16 * j;
      dst[o] = kk < ks2 ? __fmul_rn(src[(size_t)(kz * ks2 + kk) * cout + col], sc[col]) : 0.f;
    }));
  }
  if (name == "conv1" && cin == 6 && cout == 32 && K > 1) {
    // conv_cin6_quad_kernel (conv1.hip): wq[k][i][q][e] = W[k][i / 2][8 q + 4 (i % 2) + e], batch norm folded in
    const int64_t ne = (int64_t)K * 192;
    DGR_CHECK(W.alloc(&L.wq, ne));
    float *const dst = L.wq;
    DGR_CHECK(dgr_fill(s, ne, [=] __device__(int64_t o) {
      const int e = (int)(o & 3), q = (int)((o >> 2) & 3);
      const int i = (int)((o >> 4) % 12), k = (int)(o / 192);
      const int ci = i >> 1, co = 8 * q + 4 * (i & 1) + e;
      dst[o] = __fmul_rn(src[((size_t)k * cin + ci) * cout + co], sc[co]);
    }));
    W.param_bytes += (size_t)ne * sizeof(float);
  }
  W.layers.push_back(L);
  return DGR_OK;
}

static int net_create(dgr_ctx *ctx, int D, int in_channels, int out_channels, int conv1_kernel_size, int normalize_feature,
                      const dgr_weight_desc *weights, int n_weights, dgr_net **out, bool dev) {
  DGR_REQUIRE(ctx && weights && out, "dgr_net_create: NULL argument");
  if (dev) {
    // every tensor must really live on this context's device: the fill kernels dereference the pointers
    for (int i = 0; i < n_weights; ++i) {
      hipPointerAttribute_t at;
      const hipError_t e = hipPointerGetAttributes(&at, weights[i].data);
      if (e != hipSuccess) (void)hipGetLastError();
      DGR_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == ctx->device,
                  "dgr_net_create_device: '%s' is not a device pointer on device %d (use dgr_net_create for host tensors)",
                  weights[i].name ? weights[i].name : "?", ctx->device);
    }
  }
  DGR_REQUIRE(D == 3 || D == 6, "dgr_net_create: D=%d (ResUNetBN2C is used with D=3 and D=6)", D);
  DGR_REQUIRE(in_channels >= 1 && in_channels <= 256 && out_channels >= 1 && out_channels <= 64,
              "dgr_net_create: unsupported channel counts in=%d out=%d", in_channels, out_channels);
  DGR_REQUIRE(conv1_kernel_size % 2 == 1, "conv1 kernel size must be odd");
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  WeightPrep P{dev};
  DGR_HIP_CHECK(hipStreamCreate(&P.s));
  DGR_HIP_CHECK(hipMalloc((void **)&P.sc, 256 * sizeof(float)));
  DGR_HIP_CHECK(hipMalloc((void **)&P.mxb, sizeof(uint32_t)));
  DGR_CHECK(dgr_fill_fresh(P.sc, 256 * sizeof(float)));
  DGR_CHECK(dgr_fill_fresh(P.mxb, sizeof(uint32_t)));
  dgr_net *net = new dgr_net();
  net->ctx = ctx;
  net->W = std::make_shared<DgrWeights>();
  net->W->device = ctx->device;
  net->D = D; net->cin = in_channels; net->cout = out_channels;
  net->conv1_ks = conv1_kernel_size; net->normalize = normalize_feature;
  int k3 = 1, k1 = 1;
  for (int d = 0; d < D; ++d) { k3 *= 3; k1 *= conv1_kernel_size; }
  int rc = DGR_OK;
  for (const LayerRow &row : LAYERS)
    if (rc == DGR_OK) rc = make_layer(net, P, weights, n_weights, row, row.map == M_CONV1 ? k1 : row.map == M_IDENT ? 1 : k3);
  // the caller may free its tensors when the call returns
  if (rc == DGR_OK) rc = [&] { DGR_HIP_CHECK(hipStreamSynchronize(P.s)); return DGR_OK; }();
  if (rc != DGR_OK) {
    dgr_net_destroy(net);
    return rc;
  }
  *out = net;
  return DGR_OK;
}

extern "C" int dgr_net_create(dgr_ctx *ctx, int D, int in_channels, int out_channels,
                              int conv1_kernel_size, int normalize_feature,
                              const dgr_weight_desc *weights, int n_weights, dgr_net **out) {
  return net_create(ctx, D, in_channels, out_channels, conv1_kernel_size, normalize_feature, weights, n_weights, out, false);
}

extern "C" int dgr_net_create_device(dgr_ctx *ctx, int D, int in_channels, int out_channels,
                                     int conv1_kernel_size, int normalize_feature,
                                     const dgr_weight_desc *weights, int n_weights, dgr_net **out) {
  return net_create(ctx, D, in_channels, out_channels, conv1_kernel_size, normalize_feature, weights, n_weights, out, true);
}

extern "C" void dgr_net_destroy(dgr_net *net) {
  if (!net) return;
  delete net;   // the weights go with their last sharer (DgrWeights::~DgrWeights synchronises the device first)
}

extern "C" int dgr_net_share(dgr_ctx *ctx, const dgr_net *src, dgr_net **out) {
  DGR_REQUIRE(ctx && src && out, "dgr_net_share: NULL argument");
  DGR_REQUIRE(ctx->device == src->W->device, "dgr_net_share: the weights live on device %d, the context on device %d",
              src->W->device, ctx->device);
  dgr_net *net = new dgr_net();
  net->ctx = ctx;
  net->D = src->D; net->cin = src->cin; net->cout = src->cout;
  net->conv1_ks = src->conv1_ks; net->normalize = src->normalize;
  net->W = src->W;
  net->wide_coarse = src->wide_coarse;
  *out = net;
  return DGR_OK;
}

extern "C" int dgr_net_set_wide_coarse(dgr_net *net, int on) {
  DGR_REQUIRE(net, "dgr_net_set_wide_coarse: NULL argument");
  DGR_REQUIRE(net->D == 3 || !on, "dgr_net_set_wide_coarse: a D = 3 option (the 6-D net runs its wide layers rule-major anyway)");
  net->wide_coarse = on != 0;
  return DGR_OK;
}

extern "C" int dgr_net_sharers(const dgr_net *net) { return net ? (int)net->W.use_count() : 0; }
extern "C" int64_t dgr_net_param_bytes(const dgr_net *net) { return net ? net->W->param_bytes : 0; }
extern "C" int dgr_net_num_layers(const dgr_net *net) { return net ? (int)net->W->layers.size() : 0; }

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// ---- which kernel runs which layer: decided here and nowhere else
// The forward's environment switches, read once per process (the tests run the switched variants as references):
// DGR_OS_LISTS: every layer on neighbour tables through the list-based kernel (A/B + the bit-identity test of the
// kernels); DGR_NO_WIDE3: dgr_net_set_wide_coarse has no effect; DGR_NO_DSPLIT: a residual block's middle tensor stays f32.
struct Switches { bool os_lists, no_wide3, no_dsplit; };
static const Switches &switches() {
  static const Switches s{getenv("DGR_OS_LISTS") != nullptr, getenv("DGR_NO_WIDE3") != nullptr, getenv("DGR_NO_DSPLIT") != nullptr};
  return s;
}

// A layer's kernel map in both forms, as its LayerRow::map names it
struct MapRef { Map map; const DgrKernelMap *km; const DgrNbrTable *nbr; bool swapped; };
static MapRef map_of(const DgrMapSet &ms, Map map, int lvl_in, int lvl_out) {
  switch (map) {
    case M_CONV1: return {map, &ms.conv1, nullptr, false};
    case M_SAME: return {map, &ms.same[lvl_in], &ms.nsame[lvl_in], false};
    case M_DOWN: return {map, &ms.down[lvl_in], &ms.ndown[lvl_in], false};
    case M_UP: return {map, &ms.down[lvl_out], &ms.nup[lvl_out], true};   // the strided map with in / out swapped
    default: return {map, nullptr, nullptr, false};
  }
}

// The mode of a forward, needed before its maps exist.  With dgr_net_set_wide_coarse the 128 / 256-channel layers of the
// two coarse levels of a 3-D net on neighbour tables run on the wide rule-major kernel over lists derived from the tables
// (DGR_NO_WIDE3=1 / DGR_OS_LISTS=1: on the output-stationary kernel after all).  Their product rows are reserved by the
// host's bound of 27 pairs per INPUT voxel (the coarse levels' row counts live on the device): 27 KB per voxel --
// forwards beyond 16 GB of that stay on the output-stationary kernel.
static bool wide_coarse_mode(const dgr_net *net, bool use_nbr, int64_t N) {
  const std::vector<DgrLayer> &Ls = net->W->layers;
  return net->wide_coarse && use_nbr && !switches().no_wide3 && !switches().os_lists && !dgr_exact_f32() &&
         std::any_of(Ls.begin(), Ls.end(), [](const DgrLayer &L) { return L.wb != nullptr; }) &&
         27 * N * 256 * (int64_t)sizeof(float) <= (16ll << 30);
}

// ... and the kernel of one layer, once the maps are built: `in_ld` = row stride of its input, of at most n_in_cap rows
static Kind layer_kind(const DgrMapSet &ms, bool wide3, const DgrLayer &L, const MapRef &m, bool has_res, int64_t n_in_cap,
                       int in_ld) {
  if (m.map == M_IDENT) return K_IDENTITY;
  // FCGF conv1 (ks^3 offsets, <= 8 input channels) is fused with its neighbour search: no map for it
  if (m.map == M_CONV1 && ms.use_nbr) return K_CONV1_FUSED;
  // 3-D net on neighbour tables; in wide-coarse mode the layers with wide-kernel weights run rule-major over the tables' lists
  if (ms.use_nbr && !(wide3 && L.wb && !m.swapped && m.km->built)) {
    const bool split = L.w16b && !dgr_exact_f32();
    // dense tiles and parity classes read operand pieces straight from memory, by buffer loads that address the input
    // with 32-bit byte offsets: tensors of 2 GB and more stay on the list kernel
    const bool tiles = split && L.w16d && !switches().os_lists && dgr_fits_32bit_offsets(n_in_cap, in_ld);
    // same-stride layers with C <= 64 (the two finest levels of ResUNetBN2C): dense tiles, no pair lists
    if (tiles && m.map == M_SAME && dgr_conv_dense_supported(L.cin, L.cin_pad, L.cout)) return K_DENSE;
    // transposed convs with Cin, Cout multiples of 64: by parity class of the output rows
    if (tiles && m.map == M_UP && m.nbr->perm && !has_res && dgr_conv_up_supported(L.cin, L.cin_pad, L.cout)) return K_UP;
    return split ? K_OS : K_OS_F32;
  }
  // (Cin = 6 / 1 -- the inlier net's two input widths -- have kernels of their own: dgr_conv_small_cin, conv1.hip)
  if (!m.swapped && !has_res && L.cin <= 8 && L.cout == 32 && L.cin_pad == 8) return K_SMALL_CIN;
  return L.wb ? K_WIDE : K_RULE;
}

// Rows per workgroup and input channels per pipeline phase of the list-based output-stationary kernel, measured per layer
// shape on the benchmark's clouds (tools/r06_runs/run15-17.sh): the coarse levels have few rows and need small blocks to
// fill 256 CUs; with Cin >= 128 a phase of 128 channels halves the number of barrier-separated phases per tile, and at
// level 2 that pays for 64-row blocks (half the weight fragments through the vector-memory path); the one wide layer
// that writes level 0 (conv2_tr) is faster with 64
static int os_rows_per_block(int cin_pad, int lvl_out) { return lvl_out <= 1 ? 64 : lvl_out == 2 ? (cin_pad >= 128 ? 64 : 32) : 16; }
static int os_phase_channels(int cin_pad, int lvl_out) { return (cin_pad >= 256 || (cin_pad == 128 && lvl_out >= 2)) ? 128 : 64; }

// One recorded layer, launched: phase 1, `mid` (nullable) recorded behind it, phase 2 where the kind has one.  The
// forward and dgr_net_rerun_layer both launch through here.  clk: K_WIDE stamps its own start / end there (profiling).
static int run_layer(dgr_ctx *ctx, const dgr_net *net, int li, hipStream_t stream, hipEvent_t mid,
                     const char **kname = nullptr, unsigned long long *clk = nullptr) {
  const DgrLayer &L = net->W->layers[li];
  const LayerRun &r = net->runs[li];
  const DgrConvLaunch &a = r.launch;
  switch (r.kind) {
    case K_CONV1_FUSED:   // (allocates its search's temporaries: the one kind that cannot be replayed)
      DGR_CHECK(dgr_conv1_probe(ctx->arena, r.cm0, net->conv1_ks, a.in, a.in_ld, L.cin, L.w, L.shift, a.out, a.out_ld,
                                r.fused_pairs, stream, L.wc, kname, r.fused_amax));
      break;
    case K_SMALL_CIN:
      DGR_CHECK(dgr_conv_small_cin(a.in, a.in_ld, a.in_relu, L.cin, L.w, L.wq, L.shift, r.km, r.n_out, r.n_out_cap, a.out,
                                   a.out_ld, stream, kname));
      break;
    case K_WIDE: {
      DgrConvLaunch ac = a;
      ac.clk = clk;
      DGR_CHECK(dgr_conv_wide_launch(ac, r.split_in, L.wb, L.wb_piece, L.w_unscale, ctx->num_cus, stream, kname));
      break;
    }
    case K_RULE: DGR_CHECK(dgr_conv_launch(a, ctx->num_cus, stream, kname)); break;
    case K_IDENTITY: DGR_CHECK(dgr_conv_identity_launch(a, ctx->num_cus, stream, kname)); break;
    case K_OS_F32: case K_OS: case K_DENSE: case K_UP: DGR_CHECK(dgr_conv_os_launch(r.os, stream, kname)); break;
    default: DGR_REQUIRE(false, "layer %s: not launched yet", L.name.c_str());
  }
  if (mid) DGR_HIP_CHECK(hipEventRecord(mid, stream));   // end of the MFMA phase
  if (rule_major(r.kind))
    DGR_CHECK(dgr_reduce_rows(a.y, L.cout, r.red_ptr, r.red_pos, r.n_out, r.n_out_cap, r.split_only ? nullptr : a.out, a.out_ld,
                              L.shift, r.res, r.res_ld, r.res_relu, stream, r.split_out.planes ? &r.split_out : nullptr,
                              r.out_relu));
  return DGR_OK;
}

struct Fwd {
  dgr_ctx *ctx;
  dgr_net *net;
  hipStream_t stream;
  DgrMapSet ms;
  bool prof;
  bool wide3 = false;     // wide_coarse_mode
  float *ybuf = nullptr;  // per-pair product rows, sized for the largest layer of this forward

  // One conv through kernel `kind`: fills the layer's run record, makes the pending forms of its input, launches the
  // record.  Rule-major kinds: Y[pair] = in[pair_in] W[k] (MFMA), then out[o] = shift (+res) + sum of the row's Y rows.
  int conv(int li, Kind kind, const Tensor &in, const MapRef &m, int lvl_in, int lvl_out, const Tensor &out, const Tensor *res,
           bool l2_normalize) {
    const DgrLayer &L = net->W->layers[li];
    const DgrCoordMap &cin_map = ms.cm[lvl_in], &cout_map = ms.cm[lvl_out];
    const DgrKernelMap *km = m.km;
    LayerRun &r = net->runs[li];
    r = LayerRun();
    r.kind = kind;
    r.n_in = cin_map.n_dev; r.n_out = cout_map.n_dev; r.n_out_cap = cout_map.n_cap;
    r.K = L.K;
    DgrConvLaunch &a = r.launch;
    a.in = in.ptr; a.in_ld = in.ld; a.in_relu = in.relu;
    a.out = out.ptr; a.out_ld = out.ld;
    a.y = ybuf; a.shift = L.shift;
    a.w = L.w;
    a.cin = L.cin; a.cin_pad = L.cin_pad; a.cout = L.cout; a.cout_pad = L.cout_pad; a.K = L.K;
    a.pair_in = a.pair_out = a.tile_ptr = a.rule_ptr = nullptr;
    a.tile_desc = nullptr; a.n_rows_dev = nullptr; a.tile_bound = 0;
    DGR_REQUIRE(!out.split.planes || out.split_pending || rule_major(kind), "layer %s: only a reduction can write split rows",
                L.name.c_str());
    DGR_REQUIRE(kind == K_DENSE || (!in.dsplit_only && !out.dsplit_only), "layer %s: dense split rows outside the dense-tile kernel", L.name.c_str());
    // the default names: of the kinds whose launch reports none of its own
    const char *kname = "";
    if (kind == K_CONV1_FUSED) {
      kname = "conv1_grid_kernel";
      r.cm0 = cin_map;
      DGR_ALLOC(r.fused_pairs, ctx->arena, int32_t, 1);
      r.fused_amax = out.amax;
    } else if (on_tables(kind)) {
      // D = 3: output-stationary fused conv over the dense neighbour table of this (in map, out map) pair
      kname = "sparse_conv_os";
      DGR_REQUIRE(m.nbr && m.nbr->built && L.w16, "layer %s: no neighbour table / 16x16 weights", L.name.c_str());
      DgrConvOsLaunch &o = r.os;
      o.in = in.ptr; o.in_ld = in.ld; o.in_relu = in.relu;
      o.out = out.ptr; o.out_ld = out.ld; o.out_relu = out.relu;
      o.rows_per_block = os_rows_per_block(L.cin_pad, lvl_out);
      o.phase_channels = os_phase_channels(L.cin_pad, lvl_out);
      o.w16 = L.w16; o.shift = L.shift;
      o.wb3 = L.w16b; o.piece_stride = L.w16b_piece;
      o.wbd = L.w16d;
      o.w_unscale = L.w_unscale; o.n_in_cap = cin_map.n_cap;
      if (reads_amax(kind)) {
        DGR_REQUIRE(in.amax, "layer %s: the split-operand kernels need the input rows' maxima", L.name.c_str());
        o.row_amax = in.amax;
      }
      o.out_amax = out.amax; o.out_amax2 = out.amax2;
      o.res = res ? res->ptr : nullptr; o.res_ld = res ? res->ld : 0; o.res_relu = res ? res->relu : 0;
      r.nbr = *m.nbr;
      o.nbr = &r.nbr; o.n_out_dev = cout_map.n_dev; o.n_out_cap = cout_map.n_cap;
      o.cin = L.cin; o.cin_pad = L.cin_pad; o.cout = L.cout;
      o.dense = kind == K_DENSE;
      o.up = kind == K_UP;
      if (o.dense) {
        o.in_dsplit = in.dsplit;
        o.out_dsplit = out.dsplit;
        if (out.dsplit_only) o.out = nullptr;
      }
    } else if (kind == K_IDENTITY) {
      DGR_REQUIRE(res == nullptr, "identity conv with residual not supported");
      a.n_rows_dev = cout_map.n_dev;
      a.tile_bound = dgr_ceil_div(cout_map.n_cap, DGR_TILE_M);
      a.l2_normalize = l2_normalize ? 1 : 0;
    } else {
      a.pair_in = m.swapped ? km->pair_out : km->pair_in;
      a.pair_out = m.swapped ? km->pair_in : km->pair_out;
      a.tile_ptr = km->tile_ptr; a.rule_ptr = km->rule_ptr; a.tile_desc = km->tile_desc;
      a.tile_bound = km->pair_cap / DGR_TILE_M + km->K;
      DGR_REQUIRE(km->K == L.K, "layer %s: kernel volume mismatch", L.name.c_str());
      DGR_REQUIRE(!m.swapped || km->in_ptr, "layer %s: map has no in-major CSR", L.name.c_str());
      DGR_REQUIRE(kind != K_WIDE || in.split.planes, "layer %s: the wide-layer kernel needs its input as split rows", L.name.c_str());
      r.km = *km;
      r.rule_ptr = km->rule_ptr;
      r.split_in = kind == K_WIDE ? in.split : DgrSplitRows();
      r.red_ptr = m.swapped ? km->in_ptr : km->out_ptr;
      r.red_pos = m.swapped ? km->in_pos : km->out_pos;
      r.res = res ? res->ptr : nullptr; r.res_ld = res ? res->ld : 0; r.res_relu = res ? res->relu : 0;
      r.split_out = out.split;
      r.split_only = out.split_only;
      r.out_relu = out.relu;
    }
    hipEvent_t e0 = nullptr, em = nullptr, e1 = nullptr;
    unsigned long long *clk = nullptr;
    if (prof) {
      e0 = ctx->events.next(); em = ctx->events.next(); e1 = ctx->events.next();
      if (!e0 || !em || !e1) return DGR_EHIP;
      DGR_HIP_CHECK(hipEventRecord(e0, stream));
    }
    // the forms of the input that its producer could not leave, made in front of the launch (and not replayed with it)
    if (reads_amax(kind) && in.amax_pending)   // (a reduction leaves no row maxima behind)
      DGR_CHECK(dgr_row_amax(in.ptr, in.ld, L.cin, in.relu, cin_map.n_dev, cin_map.n_cap, in.amax, stream));
    if (kind == K_WIDE && in.split_pending)    // (an output-stationary kernel writes f32 rows only)
      DGR_CHECK(dgr_split_rows(in.ptr, in.ld, in.relu, cin_map.n_dev, cin_map.n_cap, in.split, stream));
    if (prof && kind == K_WIDE) {   // the kernel stamps its own start / end (dgr_ctx_conv_launch_kernel_us)
      DGR_ALLOC(clk, ctx->arena, unsigned long long, 2);
      DGR_HIP_CHECK(hipMemsetAsync(clk, 0xff, sizeof(unsigned long long), stream));       // start: atomicMin
      DGR_HIP_CHECK(hipMemsetAsync(clk + 1, 0, sizeof(unsigned long long), stream));      // end: atomicMax
    }
    DGR_CHECK(run_layer(ctx, net, li, stream, em, &kname, clk));
    if (prof) {
      DGR_HIP_CHECK(hipEventRecord(e1, stream));
      ctx->conv_spans.push_back({e0, e1});
      ctx->gemm_spans.push_back({e0, em});
      ctx->conv_kinds.push_back(kname);
      ctx->conv_clks.resize(ctx->conv_spans.size(), nullptr);
      ctx->conv_clks.back() = clk;
    }
    return DGR_OK;
  }
};

// Which forms each tensor of a forward exists in, from the layer table and the layers' kinds: what its consumers read and
// what its producer can leave behind.  Allocates them (the row maxima from ONE cleared allocation that the producers'
// epilogues fill by atomicMax: round 3 ran a row-scale pass per consuming layer, 20 launches per forward).
static int derive_forms(Fwd &f, const Kind kinds[N_LAYERS], Tensor t[N_TENSORS]) {
  DgrArena &A = f.ctx->arena;
  int producer[N_TENSORS], readers[N_TENSORS] = {};   // the layer that writes a tensor; how many read it, residuals included
  std::fill(producer, producer + N_TENSORS, -1);
  for (int li = 0; li < N_LAYERS; ++li) {
    producer[LAYERS[li].out] = li;
    readers[LAYERS[li].in]++;
    if (LAYERS[li].res != NO) readers[LAYERS[li].res]++;
  }
  for (const auto &e : INTERMEDIATES) readers[e.t]++;   // (dgr_net_get_intermediate reads f32 rows)
  bool want_amax[N_TENSORS] = {};
  // whether everything that writes into tensor i -- its producer, or those of the halves of a concatenation -- is `can`
  auto left_by = [&](int i, bool (*can)(Kind)) {
    bool any = false, all = true;
    for (int j = 0; j < N_TENSORS; ++j)
      if (TENSORS[j].buf == TENSORS[i].buf && TENSORS[j].col0 >= TENSORS[i].col0 &&
          TENSORS[j].col0 + TENSORS[j].cols <= TENSORS[i].col0 + TENSORS[i].cols && producer[j] >= 0) {
        any = true;
        all = all && can(kinds[producer[j]]);
      }
    return any && all;
  };
  int64_t amax_words = 0;
  for (int li = 0; li < N_LAYERS; ++li) {
    const int i = LAYERS[li].in;
    const int64_t rows = f.ms.cm[TENSORS[i].lvl].n_cap;
    const bool sole_reader = readers[i] == 1 && TENSORS[i].buf == i;   // not a residual, not half of a concatenation
    // split rows: iff a consumer is the wide kernel; its producer's reduction writes them, and nothing else when that
    // consumer is the only reader (the tensor between the two convs of a residual block)
    if (kinds[li] == K_WIDE && !t[i].split.planes) {
      t[i].split.channels = f.net->width((Tn)i);
      DGR_ALLOC(t[i].split.planes, A, unsigned char, (size_t)rows * 4 * t[i].split.channels);
      DGR_ALLOC(t[i].split.scale, A, float, rows);
      t[i].split_pending = !left_by(i, rule_major);
      t[i].split_only = sole_reader && !t[i].split_pending;
    }
    // row maxima: iff the layer is one of the kinds on neighbour tables or the producer's epilogue leaves them anyway;
    // pending iff the consumer really reads them (split operands) and a producer cannot leave them
    if (LAYERS[li].map != M_IDENT && (on_tables(kinds[li]) || left_by(i, writes_amax))) {
      if (!want_amax[i]) amax_words += rows;
      want_amax[i] = true;
      t[i].amax_pending = t[i].amax_pending || (reads_amax(kinds[li]) && !left_by(i, writes_amax));
    }
    // dense split rows: the middle tensor of a residual block at the two finest levels goes from dense-tile kernel to
    // dense-tile kernel: written as that kernel's operand pieces, and as nothing else
    if (!switches().no_dsplit && sole_reader && kinds[li] == K_DENSE && producer[i] >= 0 && kinds[producer[i]] == K_DENSE &&
        t[i].ld == f.net->width((Tn)i)) {
      t[i].dsplit = reinterpret_cast<unsigned char *>(t[i].ptr);
      t[i].dsplit_only = true;
    }
  }
  if (amax_words) {
    uint32_t *pool;
    DGR_ALLOC(pool, A, uint32_t, amax_words);
    DGR_HIP_CHECK(hipMemsetAsync(pool, 0, (size_t)amax_words * sizeof(uint32_t), f.stream));
    for (int i = 0; i < N_TENSORS; ++i)
      if (want_amax[i]) {
        t[i].amax = pool;
        pool += f.ms.cm[TENSORS[i].lvl].n_cap;
      }
    // both halves of a concatenation feed its row maxima, where their producers can
    for (int i = 0; i < N_TENSORS; ++i) {
      const Tn cat = TENSORS[i].buf;
      if (cat != i && t[cat].amax && left_by(i, writes_amax)) t[i].amax2 = t[cat].amax;
    }
  }
  return DGR_OK;
}

int dgr_resunet_forward_impl(dgr_ctx *ctx, dgr_net *net, const int32_t *coords, const float *feats,
                             int64_t N, float *out, hipStream_t stream) {
  DgrArena &A = ctx->arena;
  Fwd f;
  f.ctx = ctx; f.net = net; f.stream = stream; f.prof = ctx->profiling;
  hipEvent_t m0 = nullptr, m1 = nullptr;
  if (f.prof) {
    m0 = ctx->events.next(); m1 = ctx->events.next();
    DGR_HIP_CHECK(hipEventRecord(m0, stream));
  }
  f.ms.overflow = ctx->flag_dev;
  // FCGF conv1 (ks^3 offsets, <= 8 input channels) is fused with its neighbour search: no map for it (any odd kernel
  // size <= 7, also 3); such a 3-D net needs no rule-major map at all: the K = 27 layers run output-stationary over
  // dense neighbour tables (conv_os.hip).  Any other 3-D shape takes the rule-major two-phase path of conv.hip.
  const bool use_nbr = net->D == 3 && net->cin <= 8 && net->conv1_ks <= 7;
  f.wide3 = wide_coarse_mode(net, use_nbr, N);
  DGR_CHECK(dgr_build_maps(A, coords, N, net->D, net->conv1_ks, &f.ms, stream, DgrMapsMode{true, use_nbr, f.wide3}));
  if (f.prof) {
    DGR_HIP_CHECK(hipEventRecord(m1, stream));
    (net->D == 3 ? ctx->map3_spans : ctx->map6_spans).push_back({m0, m1});
  }
  const DgrMapSet &ms = f.ms;
  Kind kinds[N_LAYERS];
  MapRef maps[N_LAYERS];
  {
    // Y capacity: the largest (pair capacity x Cout) over the layers of this net that leave product rows
    // (a 3-D net on neighbour tables has lists -- and product rows -- for the maps of its wide layers only)
    int64_t need = 64;
    for (int li = 0; li < N_LAYERS; ++li) {
      const LayerRow &row = LAYERS[li];
      const DgrLayer &L = net->W->layers[li];
      maps[li] = map_of(ms, row.map, TENSORS[row.in].lvl, TENSORS[row.out].lvl);
      kinds[li] = layer_kind(ms, f.wide3, L, maps[li], row.res != NO, ms.cm[TENSORS[row.in].lvl].n_cap,
                             net->width(TENSORS[row.in].buf));
      if (rule_major(kinds[li])) need = std::max(need, maps[li].km->pair_cap * L.cout);
    }
    DGR_ALLOC(f.ybuf, A, float, need);
  }
  // activations (names follow model/resunet.py:598-649)
  Tensor t[N_TENSORS];
  // unit-norm output features (model/resunet.py:643-647): fused into the `final` conv's epilogue when a row's channels
  // fit one 32-channel block (every FCGF checkpoint of the reference: 16 or 32), else a pass of its own
  const bool fuse_l2 = net->normalize && net->cout <= 32;
  for (int i = 0; i < N_TENSORS; ++i) {
    const TensorRow &row = TENSORS[i];
    t[i].ld = net->width(row.buf);
    t[i].relu = row.relu;
    if (row.buf != i) t[i].ptr = t[row.buf].ptr + row.col0;
    else if (i == X) t[i].ptr = const_cast<float *>(feats);
    else if (i == OUT && (!net->normalize || fuse_l2)) t[i].ptr = out;
    else t[i].ptr = A.get<float>((size_t)ms.cm[row.lvl].n_cap * t[i].ld);
    if (!t[i].ptr) return DGR_ENOMEM;
  }
  DGR_CHECK(derive_forms(f, kinds, t));

  for (int li = 0; li < N_LAYERS; ++li) {
    const LayerRow &row = LAYERS[li];
    DGR_CHECK(f.conv(li, kinds[li], t[row.in], maps[li], TENSORS[row.in].lvl, TENSORS[row.out].lvl, t[row.out],
                     row.res != NO ? &t[row.res] : nullptr, fuse_l2 && row.out == OUT));
  }
  if (t[OUT].ptr != out) {
    DGR_CHECK(dgr_l2_normalize_rows(t[OUT].ptr, net->cout, out, net->cout, net->cout, 0, ms.cm[0].n_dev, ms.cm[0].n_cap, stream));
    t[OUT].ptr = out;
  }

  net->run_generation = ctx->arena.generation;
  std::copy(t, t + N_TENSORS, net->tensors);
  std::copy(ms.cm, ms.cm + 4, net->levels);
  return DGR_OK;
}

void dgr_ctx_begin_profile(dgr_ctx *ctx) {
  ctx->events.used = 0;
  ctx->conv_spans.clear();
  ctx->gemm_spans.clear();
  ctx->conv_kinds.clear();
  ctx->conv_clks.clear();
  ctx->map3_spans.clear();
  ctx->map6_spans.clear();
  ctx->conv_launches = 0;
}

int dgr_ctx_collect_profile(dgr_ctx *ctx) {
  auto total = [](const std::vector<std::pair<hipEvent_t, hipEvent_t>> &v, float *out) -> int {
    float s = 0.f, t = 0.f;
    for (auto &sp : v) {
      DGR_HIP_CHECK(hipEventElapsedTime(&t, sp.first, sp.second));
      s += t;
    }
    *out = s;
    return DGR_OK;
  };
  DGR_CHECK(total(ctx->map3_spans, &ctx->stage_ms[5]));
  DGR_CHECK(total(ctx->map6_spans, &ctx->stage_ms[6]));
  DGR_CHECK(total(ctx->conv_spans, &ctx->stage_ms[7]));
  ctx->conv_launches = (int64_t)ctx->conv_spans.size();
  ctx->conv_span_ms.clear();
  ctx->gemm_span_ms.clear();
  for (auto &sp : ctx->conv_spans) {
    float t = 0.f;
    DGR_HIP_CHECK(hipEventElapsedTime(&t, sp.first, sp.second));
    ctx->conv_span_ms.push_back(t);
  }
  for (auto &sp : ctx->gemm_spans) {
    float t = 0.f;
    DGR_HIP_CHECK(hipEventElapsedTime(&t, sp.first, sp.second));
    ctx->gemm_span_ms.push_back(t);
  }
  ctx->conv_clk_us.assign(ctx->conv_spans.size(), 0.f);
  for (size_t i = 0; i < ctx->conv_clks.size() && i < ctx->conv_clk_us.size(); ++i)
    if (ctx->conv_clks[i]) {
      unsigned long long c[2] = {0, 0};
      DGR_HIP_CHECK(hipMemcpy(c, ctx->conv_clks[i], sizeof(c), hipMemcpyDeviceToHost));
      if (c[1] > c[0]) ctx->conv_clk_us[i] = (float)((double)(c[1] - c[0]) * 0.01);   // 100-MHz ticks
    }
  return DGR_OK;
}

int dgr_flag_error(int32_t flag) {
  if (flag == 1) {
    dgr_set_error("duplicate coordinates in the sparse tensor input");
    return DGR_EINVAL;
  }
  if (flag == 2) {
    dgr_set_error("kernel-map capacity exceeded (more than the reserved pairs per output row)");
    return DGR_ENOMEM;
  }
  return DGR_OK;
}

static int check_flag(dgr_ctx *ctx, const int32_t *flag_dev, hipStream_t stream) {
  // the flag word lands in pinned host memory: the copy is asynchronous and goes in FRONT of the call's one wait (a
  // pageable destination made the copy block inside the runtime until the stream had drained, and a second
  // synchronisation followed it)
  unsigned char *pin;
  DGR_CHECK(dgr_ctx_pinned(ctx, 64, &pin));
  DGR_HIP_CHECK(hipMemcpyAsync(pin, flag_dev, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  DGR_CHECK(dgr_ctx_wait(ctx, stream));
  return dgr_flag_error(*reinterpret_cast<volatile int32_t *>(pin));
}

int dgr_ctx_new_flag(dgr_ctx *ctx, hipStream_t stream) {
  DGR_ALLOC(ctx->flag_dev, ctx->arena, int32_t, 1);
  DGR_HIP_CHECK(hipMemsetAsync(ctx->flag_dev, 0, sizeof(int32_t), stream));
  return DGR_OK;
}

int dgr_ctx_check_flag(dgr_ctx *ctx, hipStream_t stream) {
  if (!ctx->flag_dev) return DGR_OK;
  return check_flag(ctx, ctx->flag_dev, stream);
}

// the fused pipeline rewinds the arena region of a forward and reuses it: its maps / activations are gone
void dgr_net_invalidate_runs(dgr_net *net) { net->run_generation = ~0ull; }
int dgr_net_out_channels(const dgr_net *net) { return net->cout; }
int dgr_net_in_channels(const dgr_net *net) { return net->cin; }
int dgr_net_dim(const dgr_net *net) { return net->D; }
const dgr_ctx *dgr_net_ctx(const dgr_net *net) { return net->ctx; }

extern "C" int dgr_resunet_forward(dgr_ctx *ctx, dgr_net *net, const int32_t *coords, const float *feats,
                                   int64_t N, float *out, dgr_stream stream_) {
  DGR_REQUIRE(ctx && net && coords && feats && out, "dgr_resunet_forward: NULL argument");
  DGR_REQUIRE(net->ctx == ctx, "dgr_resunet_forward: the net object belongs to another context (one dgr_net per context: "
                               "dgr_net_share gives a second context its own over the same weights)");
  DGR_REQUIRE(N > 0, "dgr_resunet_forward: empty sparse tensor (N=%lld)", (long long)N);
  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DGR_CHECK(dgr_ctx_new_flag(ctx, stream));
  dgr_ctx_begin_profile(ctx);
  DGR_CHECK(dgr_resunet_forward_impl(ctx, net, coords, feats, N, out, stream));
  DGR_CHECK(dgr_ctx_check_flag(ctx, stream));  // synchronises the stream
  if (ctx->profiling) {
    memset(ctx->stage_ms, 0, sizeof(ctx->stage_ms));
    DGR_CHECK(dgr_ctx_collect_profile(ctx));
  }
  return DGR_OK;
}

// One conv layer of a network on a caller-supplied feature matrix, through exactly the kernels the forward uses for it
// (split rows + the wide-layer kernel + the reduction in the 6-D net, the output-stationary kernel in the 3-D net) over
// the same-stride 3^D kernel map of `coords`.  For layers with a 3^D kernel and Cin >= 32.  Test instrument: it lets the
// parity tests feed the split-operand kernels rows of any magnitude pattern (tests/test_gpu_split_f64.py).
extern "C" int dgr_debug_conv_layer(dgr_ctx *ctx, dgr_net *net, int layer, const int32_t *coords, const float *in,
                                    int in_relu, int64_t N, float *out, dgr_stream stream_) {
  DGR_REQUIRE(ctx && net && coords && in && out && N > 0, "dgr_debug_conv_layer: bad argument");
  DGR_REQUIRE(layer >= 0 && layer < (int)net->W->layers.size(), "layer %d out of range", layer);
  const DgrLayer &L = net->W->layers[layer];
  int k3 = 1;
  for (int d = 0; d < net->D; ++d) k3 *= 3;
  DGR_REQUIRE(L.K == k3 && L.cin >= 32, "dgr_debug_conv_layer: layer %s is not a 3^D conv with >= 32 input channels", L.name.c_str());
  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  DGR_CHECK(ctx->arena.reset());
  DGR_CHECK(dgr_ctx_new_flag(ctx, stream));
  dgr_ctx_begin_profile(ctx);
  DgrArena &A = ctx->arena;
  Fwd f;
  f.ctx = ctx; f.net = net; f.stream = stream; f.prof = false;
  f.ms.overflow = ctx->flag_dev;
  DGR_CHECK(dgr_build_maps(A, coords, N, net->D, 3, &f.ms, stream, DgrMapsMode{true, net->D == 3, false}));
  const int64_t n_cap = f.ms.cm[0].n_cap;
  if (!f.ms.use_nbr) DGR_ALLOC(f.ybuf, A, float, f.ms.same[0].pair_cap * L.cout);
  Tensor tin{const_cast<float *>(in), L.cin, in_relu}, tout{out, L.cout, 0};
  const MapRef m = map_of(f.ms, M_SAME, 0, 0);
  const Kind kind = layer_kind(f.ms, false, L, m, false, n_cap, tin.ld);
  // a tensor that did not come out of one of the conv kernels: the forms the layer reads are pending
  if (kind == K_WIDE) {
    tin.split.channels = L.cin;
    DGR_ALLOC(tin.split.planes, A, unsigned char, (size_t)n_cap * 4 * L.cin);
    DGR_ALLOC(tin.split.scale, A, float, n_cap);
    tin.split_pending = true;
  }
  if (reads_amax(kind)) {
    DGR_ALLOC(tin.amax, A, uint32_t, n_cap);
    tin.amax_pending = true;
  }
  DGR_CHECK(f.conv(layer, kind, tin, m, 0, 0, tout, nullptr, false));
  DGR_CHECK(dgr_ctx_check_flag(ctx, stream));   // synchronises the stream
  dgr_net_invalidate_runs(net);
  return DGR_OK;
}

// ---- read-back of the last forward's tensors: two entries that differ in what they call the tensors
// tensor `i` (NO: the name was not found) is there to be read
static int readable(dgr_ctx *ctx, const dgr_net *net, int i, const char *noun, const char *name) {
  DGR_REQUIRE(i > X && net->levels[TENSORS[i].lvl].n_dev, "no %s named '%s' (run a forward first)", noun, name);
  DGR_REQUIRE(net->run_generation == ctx->arena.generation,
              "the activations of the last forward are gone: a later call on this context reused its workspace");
  return DGR_OK;
}

// ... and one of its forms -- rows of rb bytes, `ld` bytes apart on the device -- comes back in the caller's row order
static int read_rows(const DgrCoordMap &cm, const void *src, size_t rb, size_t ld, void *host_out, int64_t capacity_bytes,
                     int64_t *rows) {
  int32_t n = 0;
  DGR_HIP_CHECK(hipDeviceSynchronize());
  DGR_HIP_CHECK(hipMemcpy(&n, cm.n_dev, sizeof(int32_t), hipMemcpyDeviceToHost));
  *rows = n;
  if (!host_out) return DGR_OK;
  DGR_REQUIRE(capacity_bytes >= (int64_t)n * (int64_t)rb, "host buffer too small");
  if (!cm.canon) {
    DGR_HIP_CHECK(hipMemcpy2D(host_out, rb, src, ld, rb, (size_t)n, hipMemcpyDeviceToHost));
  } else {   // rows back in first-occurrence order (coarse 6-D maps are numbered in bucket order)
    std::vector<unsigned char> tmp((size_t)n * rb);
    std::vector<int32_t> canon(n);
    DGR_HIP_CHECK(hipMemcpy2D(tmp.data(), rb, src, ld, rb, (size_t)n, hipMemcpyDeviceToHost));
    DGR_HIP_CHECK(hipMemcpy(canon.data(), cm.canon, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t p = 0; p < n; ++p) {
      DGR_REQUIRE(canon[p] >= 0 && canon[p] < n, "dgr_net_get_tensor: row numbering out of range");
      memcpy(static_cast<unsigned char *>(host_out) + (size_t)canon[p] * rb, tmp.data() + (size_t)p * rb, rb);
    }
  }
  return DGR_OK;
}

extern "C" int dgr_net_get_intermediate(dgr_ctx *ctx, dgr_net *net, const char *name, float *host_out,
                                        int64_t capacity, int64_t *rows, int64_t *cols) {
  DGR_REQUIRE(ctx && net && name && rows && cols, "NULL argument");
  int i = NO;
  for (const auto &e : INTERMEDIATES)
    if (!strcmp(name, e.name)) i = e.t;
  DGR_CHECK(readable(ctx, net, i, "intermediate", name));
  const Tensor &t = net->tensors[i];
  *cols = net->width((Tn)i);
  DGR_CHECK(read_rows(net->levels[TENSORS[i].lvl], t.ptr, (size_t)*cols * 4, (size_t)t.ld * 4, host_out, capacity * 4, rows));
  if (host_out)
    for (int64_t j = 0; j < *rows * *cols; ++j) host_out[j] = host_out[j] > 0.f ? host_out[j] : 0.f;
  return DGR_OK;
}

extern "C" int dgr_net_get_tensor(dgr_ctx *ctx, dgr_net *net, const char *name, int repr, void *host_out,
                                  int64_t capacity_bytes, int64_t *rows, int64_t *row_bytes) {
  DGR_REQUIRE(ctx && net && name && rows && row_bytes, "NULL argument");
  int i = NO;
  for (int j = 0; j < N_TENSORS; ++j)
    if (!strcmp(name, TENSORS[j].name)) i = j;
  DGR_CHECK(readable(ctx, net, i, "tensor", name));
  const Tensor &t = net->tensors[i];
  const size_t cols = (size_t)net->width((Tn)i);
  const void *src = nullptr;
  size_t rb = 0, ld = 0;   // bytes per row: returned / in memory
  const char *what = "";
  switch (repr) {
    case DGR_TENSOR_F32: src = (t.split_only || t.dsplit_only) ? nullptr : t.ptr; rb = cols * 4; ld = (size_t)t.ld * 4; what = "f32 rows"; break;
    case DGR_TENSOR_AMAX: src = t.amax; rb = ld = 4; what = "row maxima"; break;
    case DGR_TENSOR_SPLIT_PLANES: src = t.split.planes; rb = ld = cols * 4; what = "split rows"; break;
    case DGR_TENSOR_SPLIT_SCALE: src = t.split.scale; rb = ld = 4; what = "split-row scales"; break;
    case DGR_TENSOR_DENSE_SPLIT: src = t.dsplit; rb = ld = cols * 4; what = "dense split rows"; break;
    default: DGR_REQUIRE(false, "dgr_net_get_tensor: unknown representation %d", repr);
  }
  DGR_REQUIRE(src != nullptr, "the last forward did not write tensor '%s' as %s", name, what);
  *row_bytes = (int64_t)rb;
  return read_rows(net->levels[TENSORS[i].lvl], src, rb, ld, host_out, capacity_bytes, rows);
}

extern "C" int dgr_net_layer_stats(dgr_ctx *ctx, dgr_net *net, int layer, int64_t stats[8]) {
  DGR_REQUIRE(ctx && net && stats, "NULL argument");
  DGR_REQUIRE(layer >= 0 && layer < (int)net->W->layers.size(), "layer %d out of range", layer);
  const LayerRun &r = net->runs[layer];
  DGR_REQUIRE(r.n_in && r.n_out, "run a forward first");
  DGR_REQUIRE(net->run_generation == ctx->arena.generation,
              "the kernel maps of the last forward are gone: a later call on this context reused its workspace");
  const DgrLayer &L = net->W->layers[layer];
  DGR_HIP_CHECK(hipDeviceSynchronize());
  int32_t n_in = 0, n_out = 0;
  DGR_HIP_CHECK(hipMemcpy(&n_in, r.n_in, sizeof(int32_t), hipMemcpyDeviceToHost));
  DGR_HIP_CHECK(hipMemcpy(&n_out, r.n_out, sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t P = n_out, kne = 1;
  if (on_tables(r.kind)) {
    int64_t counts[27];
    DGR_CHECK(dgr_nbr_counts(r.nbr, r.n_out, counts));
    P = 0;
    kne = 0;
    for (int k = 0; k < 27; ++k) { P += counts[k]; kne += counts[k] > 0; }
  } else if (r.kind == K_CONV1_FUSED) {
    int32_t pc = 0;
    DGR_HIP_CHECK(hipMemcpy(&pc, r.fused_pairs, sizeof(int32_t), hipMemcpyDeviceToHost));
    P = pc;
    kne = r.K;
  } else if (r.rule_ptr) {
    std::vector<int32_t> rp(r.K + 1);
    DGR_HIP_CHECK(hipMemcpy(rp.data(), r.rule_ptr, (size_t)(r.K + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    P = rp[r.K];
    kne = 0;
    for (int k = 0; k < r.K; ++k) kne += rp[k + 1] > rp[k];
  }
  stats[0] = P; stats[1] = kne; stats[2] = n_in; stats[3] = n_out;
  stats[4] = L.cin; stats[5] = L.cout; stats[6] = L.K; stats[7] = 0;
  return DGR_OK;
}

// Re-run one conv layer of the last stage-wise forward `reps` times (its kernel maps and activations
// are still in the arena) and report the mean duration of phase 1 (MFMA) and phase 2 (reduce) in ms.
// Kernel-tuning instrument; not part of the inference path.
extern "C" int dgr_net_rerun_layer(dgr_ctx *ctx, dgr_net *net, int layer, int reps, float *gemm_ms, float *reduce_ms) {
  DGR_REQUIRE(ctx && net && gemm_ms && reduce_ms && reps > 0, "bad argument");
  DGR_REQUIRE(layer >= 0 && layer < (int)net->W->layers.size(), "layer %d out of range", layer);
  const LayerRun &r = net->runs[layer];
  DGR_REQUIRE(r.n_in && r.n_out, "run a forward first");
  DGR_REQUIRE(net->run_generation == ctx->arena.generation,
              "the kernel maps of the last forward are gone: a later call on this context reused its workspace");
  DGR_REQUIRE(r.kind != K_CONV1_FUSED, "layer %d ran fused with its neighbour search; not re-runnable", layer);
  // on the context's CU-masked stream if it has one (ctx->num_cus is then the share's size), else on the null stream
  hipStream_t st = ctx->part_stream;
  hipEvent_t e0, e1, e2;
  DGR_HIP_CHECK(hipEventCreate(&e0)); DGR_HIP_CHECK(hipEventCreate(&e1)); DGR_HIP_CHECK(hipEventCreate(&e2));
  float tg = 0.f, tr = 0.f;
  for (int i = 0; i < reps + 1; ++i) {  // first iteration = warm-up
    DGR_HIP_CHECK(hipEventRecord(e0, st));
    DGR_CHECK(run_layer(ctx, net, layer, st, e1));
    DGR_HIP_CHECK(hipEventRecord(e2, st));
    DGR_HIP_CHECK(hipEventSynchronize(e2));
    float a = 0.f, b = 0.f;
    DGR_HIP_CHECK(hipEventElapsedTime(&a, e0, e1));
    DGR_HIP_CHECK(hipEventElapsedTime(&b, e1, e2));
    if (i > 0) { tg += a; tr += b; }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
  *gemm_ms = tg / reps;
  *reduce_ms = tr / reps;
  return DGR_OK;
}
