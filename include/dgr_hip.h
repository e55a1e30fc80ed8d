/*
 * dgr_hip.h -- C ABI of libdgr_hip.so, the MI355X (gfx950) implementation of the
 * Deep Global Registration inference hot path.
 *
 * The reference (chrischoy/DeepGlobalRegistration) is pure Python with no FFI of
 * its own; its "operator interface" for this path is the set of Python callables
 * below.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference repo).  INTEGRATION.md shows the ctypes
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / STL types.
 *   - "dev" pointers are device (HBM) pointers valid on the ctx's device; the
 *     caller owns every input/output buffer, the library owns ctx, nets, hash
 *     tables, kernel maps and a grow-only workspace.
 *   - all work is enqueued on the caller's `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream); functions that return host scalars
 *     synchronise that stream, all others are asynchronous.
 *   - return value: DGR_OK (0) or a negative DGR_E* code; dgr_last_error()
 *     returns a thread-local message for the last failure.
 *   - a ctx is bound to one device and is not thread-safe.
 */
#ifndef DGR_HIP_H
#define DGR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dgr_ctx dgr_ctx;
typedef struct dgr_net dgr_net;
typedef struct dgr_maps dgr_maps;
typedef void *dgr_stream; /* hipStream_t */

enum {
  DGR_OK = 0,
  DGR_EINVAL = -1,   /* bad argument / shape / duplicate coordinates */
  DGR_EHIP = -2,     /* HIP runtime error */
  DGR_ENOMEM = -3,   /* workspace exhausted (kernel-map capacity overflow) */
  DGR_ESVD = -4,     /* 3x3 SVD did not converge / non-finite input: maps to the
                        RuntimeError caught at core/deep_global_registration.py:295 */
  DGR_EINTERNAL = -5
};

/* per-pair status of the confidence gate, core/deep_global_registration.py:276-281 */
enum { DGR_STATUS_OK = 0, DGR_STATUS_LOW_CONFIDENCE = 1, DGR_STATUS_SVD_FAILED = 2,
       DGR_STATUS_SAFEGUARD = 3 /* gate failed, T from the safeguard RANSAC (dgr_params.safeguard) */,
       /* flag, OR-ed onto one of the codes above (status & DGR_STATUS_MASK): dgr_params.use_icp, but the final ICP could
          not run on this pair (no finite target point); T is the estimate the code names, before ICP */
       DGR_STATUS_FLAG_ICP_SKIPPED = 0x100, DGR_STATUS_MASK = 0xff,
       /* internal: the workgroups that share a pair's refinement lost each other (never returned to the caller as a
        * status: the call fails with DGR_EINTERNAL) */
       DGR_STATUS_EXCHANGE_TIMEOUT = 0x7f };

const char *dgr_last_error(void);
const char *dgr_version(void);

/* ---- context ------------------------------------------------------------------------ */
int dgr_ctx_create(int device, dgr_ctx **out);
void dgr_ctx_destroy(dgr_ctx *ctx);
/* bytes currently reserved by the grow-only workspace (diagnostics) */
int64_t dgr_ctx_workspace_bytes(dgr_ctx *ctx);
/* A stream on its own share of the GPU's compute units (no reference counterpart: the reference registers one pair at a
 * time on torch's current stream, core/deep_global_registration.py:238-324).  A process that keeps several contexts busy
 * (one per host thread, each with its own batches) lets every kernel of every context compete for all CUs: a persistent
 * 6-D conv kernel of one context holds every CU for milliseconds and another context's 10-us launch waits behind it.
 * This call creates a stream whose kernels run on share `part` of `nparts` (2 or 4) equal shares of the CUs
 * (hipExtStreamCreateWithCUMask; mask bit b is slot b / 8 of XCD b % 8, share p takes the slots with slot % nparts == p
 * of EVERY XCD, so each share keeps all eight L2s), sizes the context's persistent launches for that share, and returns
 * the stream in *out: pass it to every entry point called with this context.  The stream belongs to the context
 * (destroyed with it; a second call replaces it after a device synchronisation).  nparts = 1 drops the partition
 * (*out = NULL).  Results do not depend on it (grids only).  Measured on MI355X, BASELINE configs[1]: four contexts on
 * four shares 396 pairs/s against 378 for three contexts on the whole GPU and 360 for four (tools/r06_runs/run42.sh). */
int dgr_ctx_create_partition_stream(dgr_ctx *ctx, int part, int nparts, dgr_stream *out);

/* ---- voxelisation: replaces ME.utils.sparse_quantize(xyz / voxel, return_index=True) and
 * ME.utils.batched_coordinates at core/deep_global_registration.py:152,158 (preprocess, :134-161).
 * xyz: dev [M,3] float64 (is_f64=1) or float32 (is_f64=0); floor(xyz/voxel) is taken in that dtype.
 * sel_out: dev int64 [>=M]   indices of the first point of every voxel, ascending
 * coords_out: dev int32 [>=M,4] (batch_index, floor(xyz[sel]/voxel))
 * xyz_out: dev float32 [>=M,3] xyz[sel] cast to float32
 * n_out: host int64*, number of voxels (synchronises the stream). */
int dgr_voxelize(dgr_ctx *ctx, const void *xyz, int is_f64, int64_t M, double voxel_size,
                 int32_t batch_index, int64_t *sel_out, int32_t *coords_out, float *xyz_out,
                 int64_t *n_out, dgr_stream stream);

/* ---- network: replaces model.load_model('ResUNetBN2C')(in, out, bn_momentum, conv1_kernel_size,
 * normalize_feature, D) + load_state_dict + .eval() (core/deep_global_registration.py:96-131;
 * class at model/resunet.py:419-665).  Tensors are HOST float32 arrays in MinkowskiEngine
 * state_dict layout ("conv1.kernel" [K,Cin,Cout], "norm1.bn.weight", ..., "final.bias");
 * the library copies them to HBM, folds eval-mode batch norm into the kernels and re-tiles them there
 * for the MFMA B-operand; the caller may free its arrays afterwards.
 * Offset axis of a kernel: index j = sum_d (delta_d + ks/2) ks^d, FIRST spatial axis fastest; a transposed
 * convolution (conv4_tr / conv3_tr / conv2_tr) pairs index and offset like the forward strided map it swaps -- the
 * library's reading of MinkowskiEngine 0.5.4 (unverifiable offline).  A checkpoint in another convention is
 * re-indexed by the caller before this call: deepglobalregistration_amd/model/me_conventions.py does it for the
 * Python host, tools/check_me_conventions.py tells the readings apart on a real pair. */
typedef struct {
  const char *name;
  const float *data; /* host (dgr_net_create) / device (dgr_net_create_device) */
  int64_t numel;
} dgr_weight_desc;

int dgr_net_create(dgr_ctx *ctx, int D, int in_channels, int out_channels, int conv1_kernel_size,
                   int normalize_feature, const dgr_weight_desc *weights, int n_weights,
                   dgr_net **out);
/* The same with every `data` a DEVICE pointer on the context's device ("host or device pointers"): the state
 * dict is already in HBM -- e.g. views of the flat RCCL broadcast buffer of a multi-GPU start (deepglobalregistration_amd/
 * dist.py) -- and is read from there, not uploaded: nothing but the per-channel batch-norm vectors (cout floats each)
 * travels to the host.  The weight preparation is dgr_net_create's: bit-identical weight sets on the same values
 * (tests/test_gpu_device_weights.py).  The library copies: the caller may free its tensors when the call returns. */
int dgr_net_create_device(dgr_ctx *ctx, int D, int in_channels, int out_channels, int conv1_kernel_size,
                          int normalize_feature, const dgr_weight_desc *weights, int n_weights,
                          dgr_net **out);
void dgr_net_destroy(dgr_net *net);
int64_t dgr_net_param_bytes(const dgr_net *net);
/* A second net object bound to `ctx` (another context of the SAME device: one context per HIP stream / host thread)
 * over the weights `src` already holds in HBM -- the equivalent of several Python threads calling one torch module in
 * the reference (core/deep_global_registration.py:96-131 builds the models once).  The weights are immutable and
 * reference-counted: they are freed when the last net sharing them is destroyed; per-forward state (kernel maps,
 * intermediates) belongs to each net object.  dgr_net_sharers: how many net objects hold `net`'s weights;
 * dgr_net_param_bytes reports the shared set's bytes (count it once per distinct weight set). */
int dgr_net_share(dgr_ctx *ctx, const dgr_net *src, dgr_net **out);
int dgr_net_sharers(const dgr_net *net);
/* D = 3 nets with at most 8 input channels (FCGF): on != 0 -- the forwards of THIS net object run the K = 27 layers with
 * 128 / 256 channels on both sides (block3, block4, block4_tr, conv4) on the wide rule-major kernel over lists derived
 * from the neighbour tables, instead of the output-stationary kernel.  Faster on the coarse levels (few rows, many pairs);
 * results agree to a few f32 ulps of a tensor's scale, not bit for bit.  Around those layers dgr_net_get_tensor then
 * serves split rows (T4, Y4, S4, T8, Y8, U4, V4; Y4, Y8, V4 as split rows only) and no row maxima for Y4, S4, T8, Y8,
 * V4.  Off (the default): every tensor as documented below.  dgr_net_share copies the setting.  DGR_NO_WIDE3=1 in the
 * environment overrides it to off. */
int dgr_net_set_wide_coarse(dgr_net *net, int on);

/* ---- sparse ResUNet forward: replaces ME.SparseTensor(feats, coordinates=coords) +
 * ResUNet2.forward (core/deep_global_registration.py:163-169, 210-217; model/resunet.py:598-649).
 * coords: dev int32 [N,1+D] (batch column first, unique rows); feats: dev f32 [N,Cin];
 * out: dev f32 [N,Cout], row i belongs to coords row i.  Asynchronous.
 * Precondition for a 3-D net with ONE input channel (the FCGF net): feats are finite numbers -- its first layer keeps
 * the input values in a dense grid whose empty cells hold the NaN bit pattern 0xffffffff, so an input with exactly those
 * bits would be read as an empty voxel (the reference feeds ones, core/deep_global_registration.py:160). */
int dgr_resunet_forward(dgr_ctx *ctx, dgr_net *net, const int32_t *coords, const float *feats,
                        int64_t N, float *out, dgr_stream stream);
/* after a forward: copy an intermediate activation ("s1","s2","s4","s8","s4_tr","s2_tr","s1_tr")
 * to a HOST buffer (post-ReLU values, like the reference's out_s* tensors); rows/cols out. */
int dgr_net_get_intermediate(dgr_ctx *ctx, dgr_net *net, const char *name, float *host_out,
                             int64_t capacity, int64_t *rows, int64_t *cols);
/* Test instrument: after a forward, copy one named tensor of it to a HOST buffer in one of the representations the
 * forward really wrote.  name: "T1" "Y1" "S1" "T2" "Y2" "S2" "T4" "Y4" "S4" "T8" "Y8" "S8" "U4" "V4" "S4T" "U2" "V2"
 * "S2T" "U1" "V1" "S1T" "H" (the activations in forward order; Y / V: the middle tensor of a residual block), the
 * concatenation buffers "CAT4" "CAT2" "CAT1" (decoder half first), and "OUT" (the caller's output buffer of that
 * forward, which must still be allocated).  repr:
 *   DGR_TENSOR_F32           f32 rows as they lie in memory: signed, the tensor's pending ReLU not applied
 *   DGR_TENSOR_AMAX          3-D net: per row one uint32, the bits of the row's largest |x| after the pending ReLU
 *   DGR_TENSOR_SPLIT_PLANES  6-D net: the split rows a wide layer gathers, 4 * channels bytes per row (per 64 channels
 *                            128 bytes of the f16 piece h, then 128 bytes of the piece m; pending ReLU applied)
 *   DGR_TENSOR_SPLIT_SCALE   ... and their power-of-two scale, one float per row: x = (h + m) / scale
 *   DGR_TENSOR_DENSE_SPLIT   3-D net: the dense split rows, 4 * channels raw bytes per row
 * A representation the forward did not write (e.g. the f32 rows of a block's middle tensor that exists as pieces only)
 * is an error, never stale memory.  Rows come back in first-occurrence order, like dgr_net_get_intermediate.
 * rows / row_bytes are always returned; host_out may be NULL to query them.  Synchronises the device. */
#define DGR_TENSOR_F32 0
#define DGR_TENSOR_AMAX 1
#define DGR_TENSOR_SPLIT_PLANES 2
#define DGR_TENSOR_SPLIT_SCALE 3
#define DGR_TENSOR_DENSE_SPLIT 4
int dgr_net_get_tensor(dgr_ctx *ctx, dgr_net *net, const char *name, int repr, void *host_out,
                       int64_t capacity_bytes, int64_t *rows, int64_t *row_bytes);
/* per-forward work statistics of the last forward (for the roofline report): for conv layer
 * `layer` (0..22): pairs, non-empty offsets, n_in, n_out, cin, cout.  Synchronises. */
int dgr_net_layer_stats(dgr_ctx *ctx, dgr_net *net, int layer, int64_t stats[8]);
int dgr_net_num_layers(const dgr_net *net);
/* kernel-tuning instrument: re-run conv layer `layer` of the last dgr_resunet_forward `reps` times on
 * the default stream and return the mean duration (ms) of its MFMA phase and its reduce phase. */
int dgr_net_rerun_layer(dgr_ctx *ctx, dgr_net *net, int layer, int reps, float *gemm_ms, float *reduce_ms);

/* ---- coordinate / kernel maps as a stand-alone object (inspection + parity tests):
 * the coordinate manager part of ME.SparseTensor / MinkowskiConvolution. */
int dgr_maps_create(dgr_ctx *ctx, const int32_t *coords, int64_t N, int D, int conv1_kernel_size,
                    dgr_maps **out, dgr_stream stream);
void dgr_maps_destroy(dgr_maps *maps);
/* coordinates of the map at tensor stride ts (1,2,4,8): host int32 [n,1+D]; returns n in *n */
int dgr_maps_get_coords(dgr_maps *maps, int ts, int32_t *host_out, int64_t capacity, int64_t *n);
/* kernel map: kind 0 = same-stride 3^D at ts, 1 = conv1 (ks^D at ts=1), 2 = strided ts -> 2ts; D = 3 only:
 * 3 / 4 / 5 = the dense neighbour tables of the output-stationary conv (same stride / ts -> 2ts / transposed
 * 2ts -> ts with out = the fine map), returned in the same (k, in, out) form.
 * host outputs: rule_ptr int32 [K+1], pair_in/pair_out int32 [P]; *K, *P returned. */
int dgr_maps_get_kernel_map(dgr_maps *maps, int kind, int ts, int32_t *rule_ptr, int64_t rule_cap,
                            int32_t *pair_in, int32_t *pair_out, int64_t pair_cap, int64_t *K,
                            int64_t *P);
/* dgr_maps_create with build flags.  DGR_MAPS_LEAN: the object is built exactly as dgr_resunet_forward builds its own
 * maps -- D = 3: the ten dense neighbour tables and nothing else (conv1 runs fused with its search); D = 6: the seven
 * rule-major maps without pair_out on the same-stride maps and with pair_k on level 0 only.  flags = 0 is
 * dgr_maps_create.  The translating getters above need pair_out: on a lean object they serve the coordinates, the
 * neighbour tables and the strided maps only. */
#define DGR_MAPS_LEAN 1
/* with DGR_MAPS_LEAN, D = 3: also what the forward of a 3-D net adds for its 128 / 256-channel layers -- lean rule-major
 * maps "same" at ts 4 and 8 and "down" at ts 4, derived from the neighbour tables (rule_ptr, pair_in, out_ptr, out_pos,
 * tile_ptr, tile_desc; no pair_out, no pair_k, no in-major CSR: the transposed conv of that map runs on "nbr_up") */
#define DGR_MAPS_NBR_LISTS 2
int dgr_maps_create_ex(dgr_ctx *ctx, const int32_t *coords, int64_t N, int D, int conv1_kernel_size, int flags,
                       dgr_maps **out, dgr_stream stream);
/* Test instrument: ONE array of a built maps object copied to the host as it lies in memory -- the library's own row
 * numbering, no translation through `canon`, no sorting.  Synchronises and copies, nothing else.
 *   kind "level"                      field "coords" int32 [n, 1+D] | "canon" int32 [n] (renumbered levels only) |
 *                                     "table" int32 [mask + 1] | scalars "n", "mask"
 *   kind "same" | "conv1" | "down"    "rule_ptr", "tile_ptr" int32 [K+1] | "tile_desc" int32 [tile_ptr[K], 4] |
 *                                     "pair_in", "pair_out", "out_pos", "in_pos" int32 [P] | "pair_k" uint16 [P] |
 *                                     "out_ptr", "in_ptr" int32 [n_cap + 1] | scalars "pair_cap", "n_cap", "K"
 *   kind "nbr_same" | "nbr_down" | "nbr_up"   "nbr" int32 [27, n_pad] | "perm" int32 [8, cls_cap] | "cls_count"
 *                                     int32 [8] | scalars "n_pad", "cls_cap"
 * (P = rule_ptr[K]; ts as in dgr_maps_get_kernel_map.)  Scalars come back as ONE int64.  *count / *elem_bytes are always
 * returned; host_out may be NULL to query them.  A map, table or field this build did not make (pair_out of a lean
 * same-stride map, in_pos of a same-stride map, canon of a level in the caller's order, ...) is DGR_EINVAL with a
 * message, never an empty or stale array. */
int dgr_maps_get_raw(dgr_maps *maps, const char *kind, int ts, const char *field, void *host_out,
                     int64_t capacity_bytes, int64_t *count, int64_t *elem_bytes);

/* ---- feature-space 1-NN: replaces core.knn.find_knn_gpu(F0, F1, nn_max_n, knn=1,
 * return_distance) (core/knn.py:23-74) incl. core.metrics.pdist (core/metrics.py:62-69).
 * F0 dev f32 [N0,C], F1 dev f32 [N1,C]; idx_out dev int64 [N0]; dist_out dev f32 [N0] or NULL.
 * squared=0: dist = sqrt(sum (a-b)^2 + 1e-7) (chunked branch, 'L2'); squared=1: sum (a-b)^2.
 * The [chunk,N1,C] temporary of the reference is never materialised. */
int dgr_knn1_l2(dgr_ctx *ctx, const float *F0, int64_t N0, const float *F1, int64_t N1, int C,
                int squared, int64_t *idx_out, float *dist_out, dgr_stream stream);

/* ---- the same search for every pair of a collated batch in ONE launch per kernel: replaces
 * core.knn.find_knn_gpu_batch(F0, F1, len_batch, ...) (core/knn.py:106-140, one find_knn_gpu call per
 * pair there).  F0 dev f32 [off0[npairs],C] / F1 dev f32 [off1[npairs],C] hold the pairs' rows back to back
 * (dataloader/base_loader.py:63-81); off0 / off1 HOST int64 [npairs+1], starting at 0, no empty pair.
 * idx_out dev int64 [off0[npairs]]: rows of the CONCATENATED F1 (the reference's `concat_results`
 * numbering, core/knn.py:131-134; subtract off1[p] for per-pair indices); dist_out as above or NULL. */
int dgr_knn1_l2_batch(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1,
                      const int64_t *off1, int npairs, int C, int squared, int64_t *idx_out,
                      float *dist_out, dgr_stream stream);

/* ---- feature-space k-NN: replaces core.knn.find_knn_gpu(F0, F1, nn_max_n > 1, knn=k, return_distance)
 * (core/knn.py:23-74, the chunked branch that honours knn).  F0 / F1 as for dgr_knn1_l2; 1 <= k <=
 * DGR_KNN_MAX_K, anything else is DGR_EINVAL.  idx_out dev int64 [N0,k], dist_out dev f32 [N0,k] or NULL,
 * row-major; row i ascending by f32 sum (a-b)^2, equal distances by the smaller index, column 0 = the
 * dgr_knn1_l2 result bit for bit (k = 1 is that call).  Columns j >= N1: index 0, distance inf (the
 * reference's repeated min on an exhausted row).  squared as for dgr_knn1_l2. */
#define DGR_KNN_MAX_K 32
int dgr_knn_l2(dgr_ctx *ctx, const float *F0, int64_t N0, const float *F1, int64_t N1, int C, int k,
               int squared, int64_t *idx_out, float *dist_out, dgr_stream stream);

/* ---- the same k-NN search for every pair of a collated batch: replaces core.knn.find_knn_gpu_batch(F0, F1,
 * len_batch, nn_max_n > 1, knn=k, ...) (core/knn.py:106-140).  F0 / F1 / off0 / off1 as for
 * dgr_knn1_l2_batch; idx_out dev int64 [off0[npairs],k]: rows of the CONCATENATED F1 (padding columns of pair p
 * hold off1[p], the reference's `concat_results` numbering); dist_out dev f32 [off0[npairs],k] or NULL. */
int dgr_knn_l2_batch(dgr_ctx *ctx, const float *F0, const int64_t *off0, const float *F1,
                     const int64_t *off1, int npairs, int C, int k, int squared, int64_t *idx_out,
                     float *dist_out, dgr_stream stream);

/* ---- 6-D inlier-network input: replaces the torch.cat at core/deep_global_registration.py:261-262
 * and inlier_feature_generation (:185-208).  idx1 dev int64 [N0] (corres_idx1; corres_idx0 is
 * arange(N0)).  feature_type 0='ones' -> feats [N0,1]; 1='coords' -> [N0,6] =
 * (cos(xyz0[i]), cos(xyz1[idx1[i]])).  coords6_out dev int32 [N0,7]. */
int dgr_inlier_inputs(dgr_ctx *ctx, const int32_t *coords0, const float *xyz0, int64_t N0,
                      const int32_t *coords1, const float *xyz1, int64_t N1, const int64_t *idx1,
                      int feature_type, int32_t *coords6_out, float *feats_out, dgr_stream stream);

/* ---- confidence gate: replaces logit.sigmoid(); weights[weights < clip] = 0; weights.sum().item()
 * (core/deep_global_registration.py:269-272).  weights_out dev f32 [N]; *wsum host (synchronises). */
int dgr_sigmoid_clip_sum(dgr_ctx *ctx, const float *logit, int64_t N, float clip, float *weights_out,
                         double *wsum, dgr_stream stream);

/* gather rows: X[i] = src[idx[i]] for [*,3] float32 (xyz1[corres_idx1] at :283-285) */
int dgr_gather_rows3(dgr_ctx *ctx, const float *src, const int64_t *idx, int64_t N, float *dst,
                     dgr_stream stream);

/* ---- weighted Procrustes: replaces core.registration.weighted_procrustes(X, Y, w, eps)
 * (core/registration.py:91-113).  X,Y dev f32 [N,3], w dev f32 [N]; R9 (row-major 3x3) and t3
 * are HOST outputs (the reference also lands on the host: .cpu() at :105,112).  3x3 SVD in f64
 * on the device.  Returns DGR_ESVD on non-finite input. */
int dgr_weighted_procrustes(dgr_ctx *ctx, const float *X, const float *Y, const float *w, int64_t N,
                            float eps, float *R9, float *t3, dgr_stream stream);

/* ---- robust SE(3) refinement: replaces core.registration.GlobalRegistration(points,
 * trans_points, weights, max_iter, max_break_count, break_threshold_ratio, quantization_size)
 * (core/registration.py:135-194) with HighDimSmoothL1Loss (core/loss.py:42-61), ortho2rotation
 * (:16-64), Adam(lr=0.1) + ExponentialLR(0.999) (:163-164): weighted-Procrustes initialisation
 * and the whole optimisation loop run in ONE persistent kernel (no per-iteration host syncs).
 * Host outputs: R9 row-major, t3, iterations, loss, break_count. */
int dgr_se3_refine(dgr_ctx *ctx, const float *X, const float *Y, const float *w, int64_t N,
                   float quantization_size, int max_iter, int max_break_count,
                   double break_threshold_ratio, float *R9, float *t3, int32_t *iterations,
                   float *loss, int32_t *break_count, dgr_stream stream);

/* ---- ICP: replaces o3d.pipelines.registration.registration_icp(source, target,
 * max_correspondence_distance = 2 * voxel, init = T) at core/deep_global_registration.py:317-322
 * (point-to-point without scaling; Open3D defaults max_iter 30, relative_fitness = relative_rmse = 1e-6).
 * src dev f32 [N0,3], dst dev f32 [N1,3]; T_init host f64[16] row-major or NULL (identity).
 * Host outputs: T_out f64[16]; stats_out f64[3] = {fitness, inlier_rmse, iterations} or NULL.  Synchronises. */
int dgr_icp_point_to_point(dgr_ctx *ctx, const float *src, int64_t N0, const float *dst, int64_t N1,
                           double max_correspondence_distance, const double *T_init, int max_iter,
                           double relative_fitness, double relative_rmse, double *T_out, double *stats_out,
                           dgr_stream stream);

/* ---- safeguard: replaces registration_ransac_based_on_correspondence(pcd0, pcd1, idx0, idx1,
 * distance_threshold, num_iterations) at core/deep_global_registration.py:50-64 (called from :302-315 when the
 * confidence gate fails): ransac_n = 4, point-to-point estimation, no checkers, every hypothesis evaluated,
 * the best 4-point hypothesis returned.  X = xyz0[idx0], Y = xyz1[idx1] dev f32 [N,3] (dgr_gather_rows3).
 * Samples come from a counter-based generator (seed) instead of Open3D's per-thread mt19937 streams and the
 * consensus test runs in f32 without fma, so that the result is reproducible (oracle/open3d_reg.py).
 * Host outputs: T_out f64[16]; stats_out f64[3] = {best hypothesis index, inlier count, inlier rmse}.  Synchronises. */
int dgr_ransac_correspondence(dgr_ctx *ctx, const float *X, const float *Y, int64_t N, double distance_threshold,
                              int64_t num_hypotheses, uint32_t seed, double *T_out, double *stats_out,
                              dgr_stream stream);

/* ---- fused pipeline: replaces DeepGlobalRegistration.register() steps 1-5 case 0
 * (core/deep_global_registration.py:248-300) for a batch of already voxelised pairs, without
 * intermediate host synchronisation.  Pair p uses rows [off0[p], off0[p+1]) of coords0/xyz0 and
 * [off1[p], off1[p+1]) of coords1/xyz1 (host offset arrays, npairs+1 entries); the batch column
 * of the coords must equal p.  Two harness-only overrides exist because no trained checkpoint is
 * available offline (both NULL in production, see DESIGN.md "Synthetic workload"):
 * override_idx1 (dev int64 [sum N0], batch-global fragment-1 row or -1 = keep) replaces 1-NN
 * results after the search ran; forced_logit (dev f32 [sum N0]) replaces the inlier network's
 * logits after it ran.
 * T_out host f32 [npairs,16] row-major 4x4, status_out host int32 [npairs],
 * stats_out host f32 [npairs,4] = (iterations, loss, break_count, wsum) or NULL. */
typedef struct {
  float clip_weight_thresh;     /* config.clip_weight_thresh, config.py:63 (0.05) */
  float voxel_size;             /* checkpoint config */
  int inlier_feature_type;      /* 0 'ones', 1 'coords' */
  int max_iter;                 /* 1000 */
  int max_break_count;          /* 20 */
  double break_threshold_ratio; /* 1e-4 as passed at :286 */
  int skip_refinement;          /* ablation (config C5): stop after weighted Procrustes */
  /* the two Open3D steps that end register() (:302-322), inside the same call (0 = leave them to the caller): */
  int safeguard;                /* pairs that fail the confidence gate: RANSAC over the putative correspondences (:302-315,
                                 * :50-64), status DGR_STATUS_SAFEGUARD; an SVD failure keeps T = identity (:295-300) */
  int64_t ransac_hypotheses;    /* 4000000 in the reference (:58) */
  uint32_t ransac_seed;
  int use_icp;                  /* point-to-point ICP from the estimate, max distance 2 voxel, 30 iterations (:317-322) */
} dgr_params;

int dgr_register_batch(dgr_ctx *ctx, dgr_net *fcgf, dgr_net *inlier, const int32_t *coords0,
                       const float *xyz0, const int64_t *off0, const int32_t *coords1,
                       const float *xyz1, const int64_t *off1, int npairs, const dgr_params *params,
                       const int64_t *override_idx1, const float *forced_logit, float *T_out,
                       int32_t *status_out,
                       float *stats_out, dgr_stream stream);
/* The same pipeline from the second stage on, for pairs of fragments whose FCGF features are already computed: the
 * "bank" is the caller's DEVICE memory, fragment f = rows bank_off[f] .. bank_off[f + 1] of bank_coords (int32 [N,4],
 * 16-byte aligned), bank_xyz (f32 [N,3]) and bank_F (f32 [N,C], 16-byte aligned, C = 16 | 32 | 64); bank_off is HOST
 * [nfrag + 1], ascending from >= 0 with no empty fragment.  pair_ids is HOST [npairs,2]: pair p registers fragment
 * pair_ids[2p] (fragment 0) onto fragment pair_ids[2p + 1] (fragment 1).  A fragment may occur any number of times, on
 * either side.  One kernel copies the rows into the concatenated layout dgr_register_batch takes (batch column = p);
 * from there on the two calls run the same code.  override_idx1 / forced_logit index that concatenation, as in
 * dgr_register_batch: rows of the concatenated fragment 1 / one value per row of the concatenated fragment 0.  The
 * library keeps nothing of the bank.  dgr_register_batch_output / _f64 serve this call like the other (which = 3, 4:
 * the gathered feature rows); stage time [0] is the gather. */
int dgr_register_pairs(dgr_ctx *ctx, dgr_net *inlier, const int32_t *bank_coords, const float *bank_xyz,
                       const float *bank_F, const int64_t *bank_off, int nfrag, int C, const int32_t *pair_ids,
                       int npairs, const dgr_params *params, const int64_t *override_idx1,
                       const float *forced_logit, float *T_out, int32_t *status_out, float *stats_out,
                       dgr_stream stream);
/* device-side intermediates of the last dgr_register_batch (valid until the next call on this
 * ctx): which = 0 idx1 (int64 [sumN0]), 1 logit (f32 [sumN0]), 2 weights (f32 [sumN0]),
 * 3 F0 (f32 [sumN0,C]), 4 F1 (f32 [sumN1,C]).  *numel receives the element count; when dst_dev is
 * not NULL the data is copied (device to device, on `stream`) into dst_dev (capacity in bytes). */
int dgr_register_batch_output(dgr_ctx *ctx, int which, void *dst_dev, int64_t capacity_bytes,
                              int64_t *numel, dgr_stream stream);
/* The transforms of the last dgr_register_batch on this context as float64, HOST [npairs,16] (what the reference's
 * register() returns, :290-291, 317-322: T is np.float64, Open3D's results are doubles).  The learned estimate is the f32
 * result widened; a pair that went through the safeguard RANSAC or the final ICP carries that stage's float64 result,
 * which dgr_register_batch's float T_out rounds.  T_out may be NULL (only *npairs is returned). */
int dgr_register_batch_f64(dgr_ctx *ctx, double *T_out, int64_t capacity_pairs, int64_t *npairs);

/* per-stage device time (ms, HIP events) of the last dgr_register_batch when profiling was
 * enabled with dgr_ctx_set_profiling(ctx, 1): [fcgf, knn, inlier_inputs, inlier_net, registration,
 * maps_3d, maps_6d, conv_kernels_total, safeguard RANSAC + ICP steps (dgr_params.safeguard / use_icp)].  Synchronises. */
int dgr_ctx_set_profiling(dgr_ctx *ctx, int enable);
#define DGR_NUM_STAGE_TIMES 9
/* writes min(capacity, DGR_NUM_STAGE_TIMES) values and the number written to *n (nullable): the explicit capacity is
 * what keeps a caller built against an older header from being overrun when the list grows. */
int dgr_ctx_stage_times_v2(dgr_ctx *ctx, float *times_ms, int capacity, int *n);
/* the version-0.1 entry point, kept under its name with its original contract: the first eight values into float[8] */
int dgr_ctx_stage_times(dgr_ctx *ctx, float *times_ms);
/* number of sparse-conv kernel launches covered by times_ms[7] */
int64_t dgr_ctx_conv_launches(dgr_ctx *ctx);
/* duration (ms) of every sparse-conv layer launch of the last profiled batch, in launch order (FCGF layers
 * 0..22, then the inlier net's): times_ms = MFMA phase + reduce phase, gemm_ms (nullable) = MFMA phase alone
 * (the sparse_conv_mfma kernel); *n = number written (<= capacity) */
int dgr_ctx_conv_launch_times(dgr_ctx *ctx, float *times_ms, float *gemm_ms, int64_t capacity, int64_t *n);
/* the same launches timed BY THE KERNEL ITSELF: execution span in microseconds (latest wave end - earliest wave start on
 * the device's 100-MHz wall clock) -- what rocprofv3 --kernel-trace reports as the kernel's duration, valid also while other
 * streams share the GPU (the HIP-event spans above then include the wait for compute units).  0 for launches whose kernel
 * is not instrumented (only the wide-layer kernel, the dominant one, is). */
int dgr_ctx_conv_launch_kernel_us(dgr_ctx *ctx, float *us, int64_t capacity, int64_t *n);
/* kernel variant that ran each of those launches (the kernel's name as rocprofv3 --kernel-trace prints it),
 * newline-separated and NUL-terminated in buf; *n = number of names written */
int dgr_ctx_conv_launch_kinds(dgr_ctx *ctx, char *buf, int64_t capacity, int64_t *n);

/* ---- measurement beside the registration path: what the reference computes on the host to judge its networks
 * (core/trainer.py:353-489, _valid_epoch).  Read-only: none of the three calls changes what dgr_register_batch computes;
 * like every top-level call they reuse the context's workspace, so fetch dgr_register_batch_output first.
 *
 * Ground-truth correspondences: replaces util.pointcloud.get_matching_indices(source, target, trans, search_voxel_size, K)
 * (util/pointcloud.py:83-96) for every pair of a collated batch in the same launches.  Pair p uses rows
 * [off0[p], off0[p+1]) of xyz0 and [off1[p], off1[p+1]) of xyz1 (dev f32 [*,3]; HOST offsets as for dgr_knn_l2_batch, but
 * a pair may be empty) and the pose T[p] (HOST f64 [npairs,16], row-major 4x4, last row ignored).  For every source row i:
 * every target row j with d^2 = |R x0[i] + t - x1[j]|^2 < radius^2, STRICTLY, in float64 on the f32 points widened
 * exactly.  Output rows (i, j), pair-local indices, ordered by i and within one i ascending by (d^2, j); with K > 0 only
 * the first K of every i (the reference's idx[:K] on Open3D's distance-sorted radius result; Open3D is absent here: the
 * strict test and the order restate KDTreeFlann.search_radius_vector_3d, ties by index are this library's).  Rows with a
 * non-finite coordinate, on either side, take no part.
 * counts_out dev int32 [off0[npairs]]: pairs of every source row (after the cap).  pairs_out dev int64 [capacity,2] or
 * NULL: NULL returns the counts and *total_out only; a capacity below the total is DGR_EINVAL, never a truncation.
 * *total_out HOST int64: pairs of the batch.  DGR_EINVAL before any device work: radius <= 0 or not finite, K < 0
 * (0 = no cap), offsets that do not start at 0 or decrease, a non-finite T.  Synchronises. */
int dgr_radius_pairs_batch(dgr_ctx *ctx, const float *xyz0, const int64_t *off0, const float *xyz1,
                           const int64_t *off1, int npairs, const double *T, double radius, int K,
                           int32_t *counts_out, int64_t *pairs_out, int64_t capacity, int64_t *total_out,
                           dgr_stream stream);
/* Correctness labels: replaces core.correspondence.find_correct_correspondence(pos_pairs, pred_pairs, hash_seed,
 * len_batch) (core/correspondence.py:14-53).  pos dev int64 [pos_off[npairs],2], pred dev int64 [pred_off[npairs],2]
 * (the pairs' lists back to back, HOST offsets), M_per_pair HOST int64 [npairs] (the reference's hash seed:
 * max(N0, N1) by default).  out dev uint8 [pred_off[npairs]]: 1 where pred[:,0] + pred[:,1] * M (wrapping int64, numpy's
 * arithmetic) occurs among the keys of the pair's positive pairs computed the same way -- np.isin on _hash, the
 * reference's collisions under a small seed included.  Synchronises. */
int dgr_pairs_isin_batch(dgr_ctx *ctx, const int64_t *pos, const int64_t *pos_off, const int64_t *pred,
                         const int64_t *pred_off, int npairs, const int64_t *M_per_pair, uint8_t *out,
                         dgr_stream stream);
/* Validation counts: replaces is_correct.sum() and the tp / fp / tn / fn bookkeeping at core/trainer.py:395, 430-437.
 * label dev uint8 [off[npairs]], weights dev f32 [off[npairs]], pred = weight > threshold (0.5 in the reference; a NaN
 * weight predicts negative), off HOST int64 [npairs+1].  counts_out HOST int64 [npairs,6] = (n, hits, tp, fp, tn, fn).
 * Integer sums only: bitwise reproducible.  Synchronises. */
int dgr_validation_counts(dgr_ctx *ctx, const uint8_t *label, const float *weights, float threshold,
                          const int64_t *off, int npairs, int64_t *counts_out, dgr_stream stream);

/* Geometric fit of registered pairs of a fragment bank (csrc/pairscore.hip): what the reference's compute_overlap_ratio
 * (util/pointcloud.py:72-80), Open3D's fitness / inlier_rmse and its GetInformationMatrixFromPointClouds are derived from.
 * bank_xyz dev f32 [N,3]; bank_off HOST [nfrag + 1], ascending from >= 0 with no empty fragment, as for dgr_register_pairs.
 * pair_ids HOST [npairs,2]: DIRECTED pairs (source fragment, target fragment); a fragment may occur any number of times on
 * either side and (i, i) is allowed.  T HOST f64 [npairs,16], row-major 4x4, maps the source into the target's frame (last
 * row ignored).  For a source row (x, y, z) (f32 widened exactly): p = ((T0 x + T1 y) + T2 z) + T3 per row of T and, for a
 * target row q, d^2 = (ex^2 + ey^2) + ez^2 with e = p - q, in float64 without fma -- the arithmetic of
 * dgr_radius_pairs_batch.  The row's PARTNER is the target row minimising (d^2, j) among those with d^2 < radius^2,
 * STRICTLY: the first entry dgr_radius_pairs_batch(K = 1) lists for the row.  Rows with a non-finite coordinate, on either
 * side, and source rows whose p is not finite take no part.
 * sums_out HOST f64 [npairs, DGR_SCORE_WIDTH], over the source rows that have a partner, summed in float64:
 *   [0] n   [1] sum d^2   [2..4] sum q (x, y, z)   [5..10] sum qx qx, qx qy, qx qz, qy qy, qy qz, qz qz
 * (a pair without any partner: eleven zeros).  One uniform grid per fragment that occurs as a target, however many pairs it
 * is the target of; no pair list is written.  Fixed-order reductions, no floating-point atomics: two runs agree bit for
 * bit, and a pair's eleven values do not depend on the other pairs of the call.  Any npairs >= 1 (launches of 65535 pairs).
 * DGR_EINVAL before any device work: a NULL argument, npairs < 1, nfrag < 1, radius <= 0 or not finite, a non-finite entry
 * in the first three rows of a T, offsets that break the bank's rules, a pair id outside [0, nfrag).  Synchronises (twice,
 * whatever npairs). */
#define DGR_SCORE_WIDTH 11
int dgr_score_pairs(dgr_ctx *ctx, const float *bank_xyz, const int64_t *bank_off, int nfrag, const int32_t *pair_ids,
                    int npairs, const double *T, double radius, double *sums_out, dgr_stream stream);

/* Robust pose-graph optimisation with line processes over the scored pairs of a scene (csrc/posegraph.hip; Choi, Zhou,
 * Koltun 2015; the step Open3D's global_optimization runs on .log + .info).  ngraphs independent graphs in one call, one
 * workgroup each.  ALL pointers are HOST pointers (a graph is a few hundred kilobytes): the library copies in, runs one
 * persistent kernel and copies out, with one synchronisation at the end.
 * Graph g has the nodes [node_off[g], node_off[g+1]) and the edges [edge_off[g], edge_off[g+1]) of the arrays (offsets
 * start at 0).  Edge e: edge_ids[e] = (s, t), node ids LOCAL to its graph; edge_T[e] = X, row-major 4x4, the pose of s in
 * t's frame (dgr_register_pairs' T of the pair (s, t); taken as rigid, last row ignored); edge_info[e] = Lambda, row-major
 * 6x6, rotation block first (dgr_score_pairs' sums through the formula at DESIGN.md 4.7); edge_uncertain[e] != 0: a loop
 * closure subject to a line process.  pose_init [N,16]: row-major 4x4, node -> common frame.
 *   E = inv(P_t) P_s inv(X),  xi = (rotation vector of E, translation of E),  chi2 = xi^T Lambda xi
 *   F*(P) = sum_certain chi2 + sum_uncertain mu chi2 / (mu + chi2)
 * minimised over the poses of every node but reference_node, which keeps its initial value bit for bit, by
 * Levenberg-Marquardt with the line processes l = (mu / (mu + chi2))^2 frozen inside an outer iteration.  It stops after
 * max_iter accepted steps, when a step lowers F* by no more than rel_tol F*, when a step's largest entry is below 1e-13,
 * or when no damping up to 1e8 yields a descent.
 * pose_out [N,16] (last rows copied from pose_init); line_out [E]: l at the final poses, 1 on certain edges;
 * stats_out [ngraphs,4] = F* of the initial poses, F* of the final poses, accepted steps, converged (1 / 0).
 * No floating-point atomics and fixed summation orders: two runs agree bit for bit, and a graph's result does not depend
 * on the other graphs of the call.
 * DGR_EINVAL before any device work: a NULL argument, ngraphs < 1, a graph without nodes or edges, more than
 * DGR_PG_MAX_NODES nodes in a graph (6 (n - 1) = 762 unknowns and a 4.6 MB normal matrix: a factorisation spread over
 * several workgroups is not implemented), an edge id outside its graph, s == t, a non-finite X (first three rows), Lambda
 * or initial pose (first three rows), mu <= 0 or not finite, a reference node outside the graph, max_iter < 0, rel_tol < 0
 * or not finite. */
#define DGR_PG_MAX_NODES 128
typedef struct {
  double mu;            /* > 0: the line-process weight */
  int reference_node;   /* the gauge: this node keeps its initial pose */
  int max_iter;         /* accepted steps at most (100 is ample) */
  double rel_tol;       /* stop when a step lowers F* by no more than rel_tol F* (1e-13) */
} dgr_pg_params;
int dgr_pose_graph_optimize(dgr_ctx *ctx, int ngraphs, const int64_t *node_off, const int64_t *edge_off,
                            const int32_t *edge_ids, const double *edge_T, const double *edge_info,
                            const uint8_t *edge_uncertain, const double *pose_init, const dgr_pg_params *params,
                            double *pose_out, double *line_out, double *stats_out, dgr_stream stream);

/* Averaging voxel down-sample of the selected fragments of a bank, each under its own pose, on ONE lattice
 * (csrc/voxelmean.hip): every occupied voxel is replaced by the mean of the points that fall into it -- Open3D's
 * voxel_down_sample, the step in front of the reference's compute_overlap_ratio (util/pointcloud.py:72-80), when one cloud
 * is given without a pose; the fused scene when all fragments of a scene are given under their optimised poses
 * (dgr_pose_graph_optimize's pose_out).  Open3D is absent here: the arithmetic below is this library's definition.
 * xyz dev [N,3], f32 or f64 (is_f64), widened exactly to float64.  off HOST [nfrag + 1], ascending strictly from >= 0 (no
 * empty fragment), as for dgr_score_pairs: fragment f is rows off[f] .. off[f+1].  frag_ids HOST [nsel]: the DISTINCT
 * fragments that take part; NULL = all fragments in order (nsel must then be nfrag).  T HOST f64 [nsel,16], row-major 4x4,
 * T[k] maps fragment frag_ids[k] into the common frame (last row ignored); NULL = no transform.  origin HOST f64 [3].
 *   transform     for a row (x, y, z): p_r = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3], r = 0..2, in float64 without fma
 *                 (the arithmetic of dgr_score_pairs); without T, p is the widened row itself
 *   quantisation  per axis u = (p - origin) / voxel_size (a correctly rounded float64 division) and c = floor(u): a point
 *                 exactly on a voxel face belongs to the voxel above it, negative coordinates use floor, not truncation.
 *                 A row takes part iff all three u are finite and -2^31 <= u < 2^31; the other rows are DROPPED and counted
 *   accumulation  per row and axis k = floor((u - c) 2^DGR_VM_FRAC_BITS), an integer in [0, 2^40]: u - c is exact except
 *                 for a negative u so small that it rounds to 1 (k = 2^40, the voxel's upper face), the scaling and the
 *                 floor are exact.  Per voxel: n = its rows, S[3] = the int64 sums of k.  Integer sums do not depend on
 *                 the order of the additions: two runs agree bit for bit, and a permutation of the rows permutes nothing
 *                 but `first`.  2^23 rows per voxel cannot overflow (short of 2^23 rows at k = 2^40).  The quantum is
 *                 2^-40 of a voxel (4.5e-14 m at 5 cm), far below the f32 inputs
 *   mean          origin + (c + (double)S / ((double)n 2^40)) voxel_size, in this order, without fma
 *   order         voxels in ascending order of their FIRST row, a row's number being its row in xyz (so the order of
 *                 frag_ids does not matter): the order dgr_voxelize gives `sel`
 * Outputs, all dev with capacity = the number of selected rows: first_out i64 [V] the first row of every voxel,
 * coords_out i32 [V,3] = c, count_out i32 [V] = n, fsum_out i64 [V,3] = S (NULL: not returned), mean_out f64 [V,3].
 * *n_out = V and *dropped_out HOST int64: writing them synchronises.  Integer atomics only, no floating-point atomics.
 * DGR_EINVAL before any device work: a NULL argument (frag_ids, T and fsum_out may be NULL), nfrag < 1, nsel < 1 (or, without
 * frag_ids, nsel != nfrag), offsets that break the bank's rules, a fragment id outside [0, nfrag) or repeated, a non-finite
 * entry in the first three rows of a T, a non-finite origin, a voxel_size that is not positive and finite, 2^31 or more
 * selected rows. */
#define DGR_VM_FRAC_BITS 40
int dgr_voxel_mean(dgr_ctx *ctx, const void *xyz, int is_f64, const int64_t *off, int nfrag, const int32_t *frag_ids,
                   int nsel, const double *T, const double *origin, double voxel_size, int64_t *first_out,
                   int32_t *coords_out, int32_t *count_out, int64_t *fsum_out, double *mean_out, int64_t *n_out,
                   int64_t *dropped_out, dgr_stream stream);

/* TSDF fusion of the depth frames of one fragment and the surface points of the fused volume (csrc/tsdf.hip): the step the
 * reference's util/integration.py takes with Open3D's ScalableTSDFVolume.  Open3D is absent here: the arithmetic below is
 * this library's own restatement of it, and tests/tsdf_ref.py is the same statement in numpy, compared bit for bit.
 * depth dev uint16 [F,H,W]; intrinsic HOST f64 [4] = (fx, fy, cx, cy), fx, fy > 0; pose HOST f64 [F,16] row-major 4x4
 * camera-to-world and extrinsic HOST f64 [F,16] = its inverse, world-to-camera, BOTH supplied by the caller (last rows
 * ignored): the library never inverts a matrix.  All geometry is float64 without fma, every step one correctly rounded
 * operation in the order written; a rigid transform M is applied per row as ((M0 x + M1 y) + M2 z) + M3.
 *   pixel        d = raw / depth_scale; the pixel is valid iff raw > 0 and d <= depth_trunc
 *   blocks       bl = voxel_length block (block = 8 or 16, sdf_trunc <= bl).  Every frame f and every pixel with v % stride
 *                == 0 and u % stride == 0 that is valid: pc = (((u - cx) / fx) d, ((v - cy) / fy) d, d), pw = pose_f pc, per
 *                axis lo = floor((pw - sdf_trunc) / bl), hi = floor((pw + sdf_trunc) / bl); a pixel with a lo < -2^26 or a
 *                hi >= 2^26 (DGR_TSDF_BLOCK_LIMIT) is skipped like an invalid one.  The pixel touches the 8 corners, bit a of
 *                the corner number choosing hi over lo on axis a, as candidate (((f Hs + vs) Ws + us) 8 + corner), Hs =
 *                ceil(H / stride), vs = v / stride.  The block list = the distinct block coordinates in ascending order of
 *                their first candidate.  No valid pixel: zero blocks, zero points, DGR_OK
 *   integration  voxel i (global integer index; block b holds i = b block + l per axis) has the centre pw = (i + 0.5)
 *                voxel_length; tsdf f32 = 0 and weight i32 = 0; the frames are applied in the order 0 .. F-1:
 *                pc = extrinsic_f pw; skip unless z > 0; uf = ((fx x) / z + cx) + 0.5, vf likewise; skip unless 0 <= uf < W
 *                and 0 <= vf < H; u = (int)uf, v = (int)vf; skip unless the pixel is valid; m = sqrt((1 + ((u - cx) / fx)^2)
 *                + ((v - cy) / fy)^2); sdf = (d - z) m; skip unless sdf > -sdf_trunc; val = min(1, sdf / sdf_trunc);
 *                tsdf = (float)(((double)tsdf weight + val) / (weight + 1)), ONE rounding to f32; weight += 1
 *   points       blocks in list order, voxels by l = (lz block + ly) block + lx, axes a = 0, 1, 2: (f0, w0) the voxel's,
 *                (f1, w1) its neighbour's at +1 along a (in the neighbouring block where need be; absent if that block is
 *                not in the list).  A point iff w0, w1 >= min_weight, -0.98f <= f0, f1 < 0.98f and (f0 < 0) != (f1 < 0):
 *                pw with pw[a] + voxel_length (|f0| / (|f0| + |f1|)) on axis a, |.| taken in float64
 * Outputs: xyz_out dev f64 [max_points,3] receives the P points.  blocks_out dev i32 [max_blocks,3], tsdf_out dev f32
 * [max_blocks, block^3], weight_out dev i32 [max_blocks, block^3]: all three or none (NULL); without them the volume lives in
 * the context's workspace.  *n_blocks_out, *n_points_out HOST: the two values the call synchronises for; *kept_out HOST
 * (NULL: not counted): the (block, frame) pairs the integration did not cull -- a frame is skipped for a whole block only
 * when no voxel of the block can pass the tests above, so the cull does not reach the result: the voxel centres lie in a
 * ball of radius sqrt(3)/2 bl around the block's centre, which extrinsic_f maps into a ball of at most max(1, the largest
 * Euclidean norm of a row of extrinsic_f's 3x3 part) times that radius around the mapped centre, and the frame is skipped
 * only when THAT ball (plus 1 % and a rounding allowance) lies wholly outside z > 0, z < depth_trunc + sdf_trunc or one of
 * the four planes through the camera that bound the image.  Poses need not be rigid: any finite pose whose inverse the
 * caller could form is accepted (scale, shear, a rotation rounded to fewer digits), and the statement holds for all of them.
 * No floating-point atomics: a voxel belongs to one thread and output positions come from scans; two runs agree bit for bit.
 * DGR_ENOMEM: the workspace cannot be grown, more blocks than max_blocks (reported before the integration) or more points
 * than max_points (nothing is written to xyz_out) -- *n_blocks_out / *n_points_out then hold what is needed; 2^31 or more
 * voxel edges.  The library never writes past a capacity.
 * DGR_EINVAL before any device work: a NULL argument (the three volume outputs and kept_out may be NULL; xyz_out only with
 * max_points = 0), F, H or W < 1, block not 8 or 16, stride < 1, min_weight < 1, voxel_length, depth_scale or depth_trunc not
 * positive and finite, sdf_trunc outside (0, bl], non-finite intrinsics, fx or fy <= 0, a non-finite entry in the first
 * three rows of a pose or an extrinsic, 2^28 or more strided pixels. */
#define DGR_TSDF_BLOCK_LIMIT 67108864
int dgr_tsdf_fragment(dgr_ctx *ctx, const uint16_t *depth, int nframes, int height, int width, const double *intrinsic,
                      const double *pose, const double *extrinsic, double voxel_length, double sdf_trunc,
                      double depth_scale, double depth_trunc, int block, int stride, int min_weight, double *xyz_out,
                      int64_t max_points, int32_t *blocks_out, float *tsdf_out, int32_t *weight_out, int64_t max_blocks,
                      int64_t *n_blocks_out, int64_t *n_points_out, int64_t *kept_out, dgr_stream stream);

/* The same fusion with colour (the reference builds its volume with color_type RGB8 and feeds it the *.color.png of every
 * depth frame): dgr_tsdf_fragment's arguments, contract and results -- blocks, tsdf, weight and the points are EXACTLY what
 * the call without colour gives -- plus color dev uint8 [F,H,W,3] (R, G, B), the same F, H, W as depth.  Open3D keeps a
 * running floating-point mean per voxel; this library keeps exact integer sums: the same mean, free of the frame order.
 * The statement is this library's own, not a claim about Open3D's roundings; tests/tsdf_color_ref.py is its numpy form.
 *   integration  every voxel carries rgb_sum i32 [3] = 0 beside tsdf / weight; whenever frame f updates the voxel's tsdf from
 *                pixel (u, v) -- the same condition, the same pixel -- rgb_sum[e] += color[f, v, u, e], e = 0, 1, 2
 *   colours      the point on edge (i0, a) with far end i1 and r = |f0| / (|f0| + |f1|), the very r that places it:
 *                m0[e] = (double)rgb_sum0[e] / (double)w0, m1 likewise; c[e] = (m0[e] + r (m1[e] - m0[e])) / 255.0, float64
 *                without fma, every step one correctly rounded operation in the order written.  w0, w1 >= min_weight >= 1.
 *                Only the two usable ends of a crossing are read: no other voxel's rgb_sum reaches an output
 * Outputs: rgb_sum_out dev i32 [max_blocks, block^3, 3] goes together with blocks_out, tsdf_out, weight_out: all four or none;
 * point_color_out dev f64 [max_points,3] in [0, 1] (NULL: not computed).  On DGR_ENOMEM for the points nothing is written to
 * point_color_out either.  The call synchronises twice, like dgr_tsdf_fragment, and adds no atomics.
 * DGR_EINVAL before any device work, beyond dgr_tsdf_fragment's: color NULL, rgb_sum_out without the other three volume
 * outputs or they without it, F > DGR_TSDF_COLOR_MAX_FRAMES (255 F must fit an int32). */
#define DGR_TSDF_COLOR_MAX_FRAMES 8421504
int dgr_tsdf_fragment_rgb(dgr_ctx *ctx, const uint16_t *depth, int nframes, int height, int width, const double *intrinsic,
                          const double *pose, const double *extrinsic, double voxel_length, double sdf_trunc,
                          double depth_scale, double depth_trunc, int block, int stride, int min_weight, double *xyz_out,
                          int64_t max_points, int32_t *blocks_out, float *tsdf_out, int32_t *weight_out, int64_t max_blocks,
                          int64_t *n_blocks_out, int64_t *n_points_out, int64_t *kept_out, const uint8_t *color,
                          int32_t *rgb_sum_out, double *point_color_out, dgr_stream stream);

/* Triangle mesh and vertex normals of a fused TSDF volume (csrc/tsdfmesh.hip): what the reference's util/integration.py gets
 * from Open3D's volume.extract_triangle_mesh().  Open3D is absent here: triangulation and roundings below are this library's
 * own statement, and tests/tsdf_mesh_ref.py is the same statement in numpy, compared bit for bit.
 * blocks dev i32 [n_blocks,3] in any order, tsdf dev f32 and weight dev i32 [n_blocks, block^3] with l = (lz block + ly) block
 * + lx: the volume dgr_tsdf_fragment returns, or one made by hand.  Voxel i is "usable" iff its block is in the list,
 * weight >= min_weight and -0.98f <= tsdf < 0.98f.  float64 without fma, every step one correctly rounded operation.
 *   vertices     exactly the points of dgr_tsdf_fragment: blocks in list order, voxels by l, axes a = 0, 1, 2; a vertex on
 *                the edge (i0, a), i1 = i0 + e_a, iff both ends are usable and (f0 < 0) != (f1 < 0); r = |f0| / (|f0| + |f1|);
 *                position (i0 + 0.5) voxel_length with + voxel_length r on axis a.  Vertex k of the mesh is point k of the
 *                fragment; a vertex no triangle uses stays in the list
 *   normals      F(j; i) = (double)tsdf[j] if voxel j exists and weight[j] >= min_weight, else (double)tsdf[i];
 *                g(i)[e] = F(i + e_e; i) - F(i - e_e; i); n[e] = g(i0)[e] + r (g(i1)[e] - g(i0)[e]) with the very r of the
 *                position; len = sqrt((n0^2 + n1^2) + n2^2); normal = n / len, (0, 0, 0) when len == 0.  It points from
 *                negative to positive, the side the triangles face.  Non-finite tsdf values are outside the contract
 *   cells        cell i has the corners i + ((c & 1), (c >> 1) & 1, (c >> 2) & 1), c = 0..7, and the place (block, l) of
 *                voxel i; it is valid iff all eight corners are usable; configuration bit c set iff tsdf[corner c] < 0
 *                (-0.0f is not negative).  Every sign-changing edge of a valid cell is a vertex
 *   triangles    blocks in list order, cells by l, the triangles of the configuration in table order (csrc/mc_table.h,
 *                generated by tools/gen_mc_table.py from the rule stated there), three vertex indices each.  Edge e = 4 a + j
 *                of a cell lies along axis a, bit 0 of j the offset on the lower other axis, bit 1 on the higher; its
 *                vertex is the one owned by the edge's low corner voxel, in up to seven other blocks.  (v1 - v0) x (v2 - v0)
 *                points to the positive side; two cells that share a face cut it alike, so the mesh is watertight
 * Outputs: xyz_out dev f64 [max_vertices,3], normal_out dev f64 [max_vertices,3] (NULL: not computed), tri_out dev i32
 * [max_triangles,3]; *n_vertices_out, *n_triangles_out HOST: the call synchronises once, for both.  n_blocks = 0: zero
 * vertices, zero triangles, DGR_OK.  No floating-point atomics, output positions come from scans: two runs agree bit for bit.
 * DGR_ENOMEM: the workspace cannot be grown; more vertices than max_vertices or more triangles than max_triangles (nothing is
 * written to either output; both out-parameters hold what is needed); 5 n_blocks block^3 >= 2^31.  The library never writes
 * past a capacity.
 * DGR_EINVAL before any device work: a NULL argument (normal_out may be NULL; blocks, tsdf, weight only with n_blocks = 0;
 * xyz_out / tri_out only with a capacity of 0), n_blocks < 0, block not 8 or 16, min_weight < 1, voxel_length not positive and
 * finite, a negative capacity.  DGR_EINVAL found on the device and reported at the synchronisation, before anything is written
 * to an output: a block coordinate outside [-2^26, 2^26) (DGR_TSDF_BLOCK_LIMIT), a block that occurs twice in the list. */
int dgr_tsdf_mesh(dgr_ctx *ctx, const int32_t *blocks, int64_t n_blocks, const float *tsdf, const int32_t *weight, int block,
                  double voxel_length, int min_weight, double *xyz_out, double *normal_out, int64_t max_vertices,
                  int32_t *tri_out, int64_t max_triangles, int64_t *n_vertices_out, int64_t *n_triangles_out,
                  dgr_stream stream);

/* The same mesh with vertex colours: dgr_tsdf_mesh's arguments, contract and results plus rgb_sum dev i32 [n_blocks, block^3, 3],
 * the colour sums dgr_tsdf_fragment_rgb returns beside tsdf / weight, and color_out dev f64 [max_vertices,3]: the colour of
 * vertex k by the formula stated at dgr_tsdf_fragment_rgb -- point k's colour there, the same bits (one text computes both).
 * Only the rgb_sum of the two usable ends of a crossing is read.  Nothing is written to color_out on DGR_ENOMEM or on an
 * error found on the device.  DGR_EINVAL before any device work, beyond dgr_tsdf_mesh's: rgb_sum NULL with n_blocks > 0,
 * color_out NULL with max_vertices > 0. */
int dgr_tsdf_mesh_rgb(dgr_ctx *ctx, const int32_t *blocks, int64_t n_blocks, const float *tsdf, const int32_t *weight, int block,
                      double voxel_length, int min_weight, double *xyz_out, double *normal_out, int64_t max_vertices,
                      int32_t *tri_out, int64_t max_triangles, int64_t *n_vertices_out, int64_t *n_triangles_out,
                      const int32_t *rgb_sum, double *color_out, dgr_stream stream);

/* ---- debug entry points (parity tests): the device functions of the registration kernel on their own.
 * ortho2rotation (core/registration.py:16-64) forward for n parameter rows p6 [n,6] -> R9_out [n,9] (row-major 3x3) and,
 * when grad_R9 [n,9] and grad_p6_out [n,6] are given, its backward (what autograd computes for sum(R * grad_R)).
 * All pointers are device pointers. */
int dgr_debug_ortho2rotation(dgr_ctx *ctx, const float *p6, int64_t n, const float *grad_R9, float *R9_out,
                             float *grad_p6_out, dgr_stream stream);
/* The refinement loop of dgr_se3_refine (core/registration.py:168-190) RESUMED at iteration state_in[27] from a given
 * optimiser state and run up to iteration max_iter: 30 HOST doubles = prm[9] (rot6d, trans), Adam exp_avg[9],
 * exp_avg_sq[9], iteration, loss_prev, break count; state_out receives the state it ends with.  X, Y, w as for
 * dgr_se3_refine (device).  Parity instrumentation: lets a test run W steps of this kernel and W steps of the reference
 * algorithm (in f32 and in f64) from the SAME state, so that the comparison does not pass through the chaotic
 * amplification of a whole trajectory. */
int dgr_debug_se3_refine_from(dgr_ctx *ctx, const float *X, const float *Y, const float *w, int64_t N,
                              float quantization_size, int max_iter, int max_break_count,
                              double break_threshold_ratio, const double *state_in, double *state_out,
                              dgr_stream stream);
/* HighDimSmoothL1Loss (core/loss.py:51-61) per point of X, Y [n,3] (device) with quantization_size q -> per_point_out [n] */
int dgr_debug_smooth_l1(dgr_ctx *ctx, const float *X, const float *Y, int64_t n, float quantization_size,
                        float *per_point_out, dgr_stream stream);

/* One conv layer (index in forward order, 0..22; layers with a 3^D kernel and >= 32 input channels) of `net` applied to
 * a caller-supplied feature matrix `in` [N, Cin] (device; max(x, 0) applied first when in_relu) over the same-stride
 * 3^D kernel map of `coords` [N, 1+D]: out [N, Cout] (device) = folded batch-norm shift + sum over the map, through the
 * very kernels the forward runs for that layer (model/residual_block.py:118-134; MinkowskiConvolution.forward). */
int dgr_debug_conv_layer(dgr_ctx *ctx, dgr_net *net, int layer, const int32_t *coords, const float *in, int in_relu,
                         int64_t N, float *out, dgr_stream stream);

/* Test instrument of the DGR_WORKSPACE_FILL=<32-bit hex word> switch (read once per process; when set, every private device
 * allocation of the library and the context's workspace at the start of every call hold that word): resets the context's
 * workspace, takes nwords 32-bit words from its start, writes nothing to them and copies them to host_out [nwords] (HOST).
 * Synchronises the device. */
int dgr_debug_workspace_peek(dgr_ctx *ctx, int64_t nwords, uint32_t *host_out);

/* Test instrument: the route trace of the feature-space k-NN searches.  Off by default, and then a search issues exactly
 * the launches and copies it always did.  On (enable != 0): after every prefiltered descriptor table of a k-NN call on
 * this context -- dgr_knn1_l2 / dgr_knn_l2, their _batch forms, and the search inside dgr_register_batch /
 * dgr_register_pairs -- the library waits for the stream and reduces the table's per-pair words and candidate counts
 * on the host.  Switching clears the recorded rows. */
int dgr_ctx_set_knn_trace(dgr_ctx *ctx, int enable);
/* One row of 8 int32 per pair of the last traced k-NN call, in call order, into host_out [capacity_rows][8] (HOST; at
 * most capacity_rows rows are written, NULL allowed with capacity_rows == 0); *nrows = the rows the call recorded.
 * Fields: pair index in the call; descriptor table (32 pairs each); route, 0 = brute force (C = 16 / 64, a small
 * reference set, DGR_KNN_BRUTE), 1 = bf16 prefilter; then, for route 1 (0 otherwise): fallback flag (non-finite / huge
 * input), length of the overflow list, redo-by-brute-force flag, largest candidate count over the pair's queries,
 * number of its queries without a candidate. */
int dgr_debug_knn_trace(dgr_ctx *ctx, int32_t *host_out, int64_t capacity_rows, int64_t *nrows);

#ifdef __cplusplus
}
#endif
#endif /* DGR_HIP_H */
