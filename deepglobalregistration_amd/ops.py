"""Thin torch-tensor wrappers over the C ABI (one function per entry point of
include/dgr_hip.h).  torch supplies device memory and the current stream only; all
arithmetic happens in libdgr_hip.so."""
import ctypes as C

import numpy as np
import torch

from . import _args, _lib
from ._lib import check, get_ctx, ptr, stream_ptr, vp

F32_EPS = float(np.finfo(np.float32).eps)

_NP_PTR = {np.dtype(np.int32): _lib.c_i32p, np.dtype(np.int64): _lib.c_i64p, np.dtype(np.float32): _lib.c_f32p,
           np.dtype(np.float64): _lib.c_f64p, np.dtype(np.uint8): C.POINTER(C.c_uint8)}


def _np_ptr(a):
    """Typed pointer to a contiguous host array of one of the dtypes the C ABI takes (None -> NULL); the pointer type
    follows the array's own dtype, so the prototype refuses an array of the wrong one."""
    return None if a is None else a.ctypes.data_as(_NP_PTR[a.dtype])


def _dev(t):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError('expected a CUDA(ROCm) tensor')
    return t.device


def _as(t, dtype, device):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    return t.to(device=device, dtype=dtype).contiguous()


# ----------------------------------------------------------------------------
def voxelize(xyz, voxel_size, batch_index=0, device='cuda'):
    """ME.utils.sparse_quantize(xyz / voxel, return_index=True) + batched_coordinates
    (core/deep_global_registration.py:152-158).  Returns (xyz_sel f32 [N,3], coords i32 [N,4],
    sel i64 [N]) on the device.  float64 input is quantised in float64 like the reference."""
    lib = _lib.load()
    device = torch.device(device)
    if not torch.is_tensor(xyz):
        xyz = torch.from_numpy(np.ascontiguousarray(xyz))
    if xyz.dtype not in (torch.float32, torch.float64):
        xyz = xyz.double()
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f'expected an [M,3] point array, got {tuple(xyz.shape)}')
    xyz = xyz.to(device).contiguous()
    M = xyz.shape[0]
    if M == 0:
        raise ValueError('empty point cloud')
    sel = torch.empty(M, dtype=torch.int64, device=device)
    coords = torch.empty((M, 4), dtype=torch.int32, device=device)
    out = torch.empty((M, 3), dtype=torch.float32, device=device)
    n = C.c_int64(0)
    check(lib.dgr_voxelize(get_ctx(device), ptr(xyz), int(xyz.dtype == torch.float64), M,
                           float(voxel_size), int(batch_index), ptr(sel), ptr(coords), ptr(out),
                           C.byref(n), stream_ptr(device.index)))
    n = n.value
    return out[:n], coords[:n], sel[:n]


# ----------------------------------------------------------------------------
class NetHandle:
    """Owns a dgr_net (weights resident in HBM).  The state dict must already be in the library's kernel-offset
    convention (include/dgr_hip.h at dgr_net_create; model/me_conventions.py converts a checkpoint written under
    another reading -- `ResUNet2.load_state_dict` does that, this class and the C API do not)."""

    def __init__(self, state_dict, D, in_channels, out_channels, conv1_kernel_size,
                 normalize_feature, device='cuda', share_from=None, wide_coarse=False):
        # wide_coarse (D = 3): dgr_net_set_wide_coarse -- the coarse levels' 128 / 256-channel layers on the wide kernel
        lib = _lib.load()
        self.wide_coarse = bool(wide_coarse)
        self.device = torch.device(device)
        self.D, self.cin, self.cout = D, in_channels, out_channels
        self.conv1_ks, self.normalize = int(conv1_kernel_size), bool(normalize_feature)
        if share_from is not None:
            # a net object for the calling thread's context over the weights `share_from` already holds (dgr_net_share)
            if (share_from.D, share_from.cin, share_from.cout, share_from.conv1_ks, share_from.normalize) != \
                    (D, in_channels, out_channels, self.conv1_ks, self.normalize):
                raise ValueError('share_from is a different network')
            h = vp()
            with torch.cuda.device(self.device):
                check(lib.dgr_net_share(get_ctx(self.device), share_from.handle, C.byref(h)))
            self.handle = h
            check(lib.dgr_net_set_wide_coarse(h, int(self.wide_coarse)))
            return
        keep, descs = [], []
        items = [(n, t) for n, t in state_dict.items() if not n.endswith('num_batches_tracked')]
        # a state dict that is ALREADY on this device (torch CUDA tensors: e.g. views of the broadcast buffer of a
        # multi-GPU start, dist.broadcast_checkpoint) stays there: dgr_net_create_device reads it in place; anything
        # else goes through dgr_net_create, which uploads it first
        on_device = bool(items) and all(torch.is_tensor(t) and t.is_cuda and t.device.index == (self.device.index or 0)
                                        for _, t in items)
        self.created_on_device = on_device
        for name, t in items:
            if on_device:
                a = t.detach().to(torch.float32).contiguous()
                keep.append(a)
                descs.append(_lib.WeightDesc(name.encode(), a.data_ptr(), a.numel()))
            else:
                a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
                a = np.ascontiguousarray(a, dtype=np.float32)
                keep.append(a)
                descs.append(_lib.WeightDesc(name.encode(), a.ctypes.data, a.size))
        arr = (_lib.WeightDesc * len(descs))(*descs)
        h = vp()
        with torch.cuda.device(self.device):
            if on_device:
                torch.cuda.current_stream(self.device).synchronize()   # the tensors' producers (a broadcast) have finished
            create = lib.dgr_net_create_device if on_device else lib.dgr_net_create
            check(create(get_ctx(self.device), D, in_channels, out_channels,
                         conv1_kernel_size, int(bool(normalize_feature)), arr, len(descs),
                         C.byref(h)))
        self.handle = h
        if self.wide_coarse:
            check(lib.dgr_net_set_wide_coarse(h, 1))

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                _lib.load().dgr_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    @property
    def param_bytes(self):
        return _lib.load().dgr_net_param_bytes(self.handle)

    @property
    def sharers(self):
        """Net objects (one per context) that hold this net's weight set."""
        return _lib.load().dgr_net_sharers(self.handle)

    def forward(self, coords, feats):
        lib = _lib.load()
        dev = self.device
        coords = _as(coords, torch.int32, dev)
        feats = _as(feats, torch.float32, dev)
        if coords.dim() != 2 or coords.shape[1] != self.D + 1:
            raise ValueError(f'coords must be [N,{self.D + 1}] (batch column first), got {tuple(coords.shape)}')
        if feats.dim() != 2 or feats.shape != (coords.shape[0], self.cin):
            raise ValueError(f'feats must be [{coords.shape[0]},{self.cin}], got {tuple(feats.shape)}')
        N = coords.shape[0]
        if N == 0:
            raise ValueError('empty sparse tensor')
        out = torch.empty((N, self.cout), dtype=torch.float32, device=dev)
        check(lib.dgr_resunet_forward(get_ctx(dev), self.handle, ptr(coords), ptr(feats), N, ptr(out),
                                      stream_ptr(dev.index)))
        return out

    def intermediate(self, name):
        lib = _lib.load()
        rows, cols = C.c_int64(0), C.c_int64(0)
        ctx = get_ctx(self.device)
        check(lib.dgr_net_get_intermediate(ctx, self.handle, name.encode(), None, 0, C.byref(rows), C.byref(cols)))
        buf = np.empty((rows.value, cols.value), np.float32)
        check(lib.dgr_net_get_intermediate(ctx, self.handle, name.encode(), buf.ctypes.data, buf.size,
                                           C.byref(rows), C.byref(cols)))
        return buf

    TENSOR_REPRS = {'f32': (0, np.float32), 'amax': (1, np.uint32), 'split_planes': (2, np.uint8),
                    'split_scale': (3, np.float32), 'dense_split': (4, np.uint8)}

    def tensor(self, name, repr='f32'):
        """Named tensor `name` of the last forward in representation `repr` (dgr_net_get_tensor; test instrument):
        'f32' [n, C] signed rows, 'amax' [n] uint32, 'split_planes' [n, 4 C] bytes, 'split_scale' [n], 'dense_split'
        [n, 4 C] bytes.  Raises if the forward did not write that representation."""
        lib = _lib.load()
        code, dtype = self.TENSOR_REPRS[repr]
        rows, rb = C.c_int64(0), C.c_int64(0)
        ctx = get_ctx(self.device)
        check(lib.dgr_net_get_tensor(ctx, self.handle, name.encode(), code, None, 0, C.byref(rows), C.byref(rb)))
        buf = np.empty((rows.value, rb.value // np.dtype(dtype).itemsize), dtype)
        check(lib.dgr_net_get_tensor(ctx, self.handle, name.encode(), code, buf.ctypes.data, buf.nbytes,
                                     C.byref(rows), C.byref(rb)))
        return buf[:, 0] if repr in ('amax', 'split_scale') else buf

    def debug_conv_layer(self, layer, coords, feats, relu=False):
        """Conv layer `layer` (forward order) applied to `feats` [N, Cin] over the 3^D same-stride map of `coords`,
        through the kernels the forward uses for it (dgr_debug_conv_layer; test instrument)."""
        dev = self.device
        coords = _as(coords, torch.int32, dev)
        feats = _as(feats, torch.float32, dev)
        lay = _lib.load()
        st_cout = None
        # the layer's output width: the channel tables of ResUNetBN2C (model/resunet.py:664-665)
        ch, tr = [None, 32, 64, 128, 256], [None, 64, 64, 64, 128]
        widths = [ch[1]] * 3 + [ch[2]] * 3 + [ch[3]] * 3 + [ch[4]] * 3 + [tr[4]] * 3 + [tr[3]] * 3 + [tr[2]] * 3 + [tr[1], self.cout]
        st_cout = widths[layer]
        out = torch.empty((coords.shape[0], st_cout), dtype=torch.float32, device=dev)
        check(lay.dgr_debug_conv_layer(get_ctx(dev), self.handle, int(layer), ptr(coords), ptr(feats), int(bool(relu)),
                                       coords.shape[0], ptr(out), stream_ptr(dev.index)))
        return out

    def rerun_layer(self, layer, reps=5):
        """(gemm_ms, reduce_ms) of conv layer `layer` of the last forward (kernel-tuning instrument)."""
        lib = _lib.load()
        g, r = C.c_float(0), C.c_float(0)
        check(lib.dgr_net_rerun_layer(get_ctx(self.device), self.handle, layer, reps, C.byref(g), C.byref(r)))
        return g.value, r.value

    def layer_stats(self):
        """Per conv layer of the last forward: dict(pairs, nonempty, n_in, n_out, cin, cout, K)."""
        lib = _lib.load()
        out = []
        for li in range(lib.dgr_net_num_layers(self.handle)):
            st = (C.c_int64 * 8)()
            check(lib.dgr_net_layer_stats(get_ctx(self.device), self.handle, li, st))
            out.append(dict(pairs=st[0], nonempty=st[1], n_in=st[2], n_out=st[3], cin=st[4], cout=st[5], K=st[6]))
        return out


# ----------------------------------------------------------------------------
class Maps:
    """Coordinate maps + kernel maps of one sparse tensor (inspection / parity tests).  lean=True builds the object
    exactly as a network forward builds its own maps (dgr_maps_create_ex, DGR_MAPS_LEAN); nbr_lists=True (lean, D = 3)
    adds the rule-major lists the forward of a 3-D net derives from its neighbour tables for its 128 / 256-channel
    layers (DGR_MAPS_NBR_LISTS: 'same' at ts 4 and 8, 'down' at ts 4)."""

    def __init__(self, coords, D, conv1_kernel_size=3, device='cuda', lean=False, nbr_lists=False):
        lib = _lib.load()
        self.device = torch.device(device)
        coords = _as(coords, torch.int32, self.device)
        self.D, self.lean = D, bool(lean)
        h = vp()
        if lean:
            check(lib.dgr_maps_create_ex(get_ctx(self.device), ptr(coords), coords.shape[0], D, conv1_kernel_size,
                                         1 | (2 if nbr_lists else 0), C.byref(h), stream_ptr(self.device.index)))
        elif nbr_lists:
            raise ValueError('nbr_lists goes with lean=True')
        else:
            check(lib.dgr_maps_create(get_ctx(self.device), ptr(coords), coords.shape[0], D, conv1_kernel_size,
                                      C.byref(h), stream_ptr(self.device.index)))
        self.handle = h

    def raw(self, kind, ts, field):
        """One array of the object as it lies in device memory (dgr_maps_get_raw; test instrument): the library's own
        row numbering, nothing translated or sorted.  kind 'level' | 'same' | 'conv1' | 'down' | 'nbr_same' | 'nbr_down'
        | 'nbr_up'; scalars come back as int.  A field the build did not make raises ValueError."""
        lib = _lib.load()
        n, eb = C.c_int64(0), C.c_int64(0)
        check(lib.dgr_maps_get_raw(self.handle, kind.encode(), ts, field.encode(), None, 0, C.byref(n), C.byref(eb)))
        scalar = eb.value == 8
        buf = np.empty(n.value, np.int64 if scalar else np.uint16 if eb.value == 2 else np.int32)
        check(lib.dgr_maps_get_raw(self.handle, kind.encode(), ts, field.encode(), buf.ctypes.data, buf.nbytes,
                                   C.byref(n), C.byref(eb)))
        if scalar:
            return int(buf[0])
        shape = {'coords': (-1, self.D + 1), 'tile_desc': (-1, 4), 'nbr': (27, -1), 'perm': (8, -1)}.get(field)
        return buf.reshape(shape) if shape else buf

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                _lib.load().dgr_maps_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def coords(self, ts):
        lib = _lib.load()
        n = C.c_int64(0)
        check(lib.dgr_maps_get_coords(self.handle, ts, None, 0, C.byref(n)))
        out = np.empty((n.value, self.D + 1), np.int32)
        check(lib.dgr_maps_get_coords(self.handle, ts, out.ctypes.data, out.size, C.byref(n)))
        return out

    def kernel_map(self, kind, ts):
        """kind: 'same' | 'conv1' | 'down' (rule-major maps) or, D = 3 only, 'nbr_same' | 'nbr_down' | 'nbr_up'
        (the dense neighbour tables of the output-stationary conv; 'nbr_up' = transposed conv 2 ts -> ts).
        Returns (k, in, out) int64 arrays sorted by (k, out)."""
        lib = _lib.load()
        kid = {'same': 0, 'conv1': 1, 'down': 2, 'nbr_same': 3, 'nbr_down': 4, 'nbr_up': 5}[kind]
        K, P = C.c_int64(0), C.c_int64(0)
        check(lib.dgr_maps_get_kernel_map(self.handle, kid, ts, None, 0, None, None, 0, C.byref(K), C.byref(P)))
        rule = np.empty(K.value + 1, np.int32)
        pin = np.empty(P.value, np.int32)
        pout = np.empty(P.value, np.int32)
        check(lib.dgr_maps_get_kernel_map(self.handle, kid, ts, rule.ctypes.data, rule.size, pin.ctypes.data,
                                          pout.ctypes.data, pin.size, C.byref(K), C.byref(P)))
        k = np.repeat(np.arange(K.value), np.diff(rule))
        return k.astype(np.int64), pin.astype(np.int64), pout.astype(np.int64)


# ----------------------------------------------------------------------------
KNN_MAX_K = 32   # DGR_KNN_MAX_K of include/dgr_hip.h


def check_knn_k(k):
    """The k of a k-NN search as an int in [1, KNN_MAX_K]; ValueError otherwise (before any device work)."""
    # (not _args.integer: the range message prints int(k), the type message k itself)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError(f'knn must be an integer in [1, {KNN_MAX_K}], got {k!r}')
    if not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError(f'knn must be an integer in [1, {KNN_MAX_K}], got {int(k)}')
    return int(k)


def _knn(F0, F1, off0, off1, k, squared, return_distance):
    """The four k-NN searches.  off0 / off1 None: one pair (F0 against F1), otherwise the batched entry points; k None:
    the 1-NN entry points, which write idx [N0] where the k-NN ones (k from `check_knn_k`) write [N0,k]."""
    lib = _lib.load()
    dev = _dev(F0)
    F0 = _as(F0, torch.float32, dev)
    F1 = _as(F1, torch.float32, dev)
    if F0.dim() != 2 or F1.dim() != 2 or F0.shape[1] != F1.shape[1]:
        raise ValueError('F0 [N0,C] and F1 [N1,C] must share the feature width')
    N0, N1 = F0.shape[0], F1.shape[0]
    if off0 is None:
        fn = lib.dgr_knn1_l2 if k is None else lib.dgr_knn_l2
        sides = (ptr(F0), N0, ptr(F1), N1)
    else:
        o0 = np.ascontiguousarray(off0, dtype=np.int64)
        o1 = np.ascontiguousarray(off1, dtype=np.int64)
        if len(o0) != len(o1) or len(o0) < 2 or o0[0] != 0 or o1[0] != 0 or o0[-1] != N0 or o1[-1] != N1:
            raise ValueError('off0 / off1 must be [npairs+1] row offsets covering F0 / F1')
        fn = lib.dgr_knn1_l2_batch if k is None else lib.dgr_knn_l2_batch
        sides = (ptr(F0), _np_ptr(o0), ptr(F1), _np_ptr(o1), len(o0) - 1)
    idx = torch.empty(N0 if k is None else (N0, k), dtype=torch.int64, device=dev)
    dist = torch.empty(idx.shape, dtype=torch.float32, device=dev) if return_distance else None
    check(fn(get_ctx(dev), *sides, F0.shape[1], *(() if k is None else (k,)), int(squared), ptr(idx), ptr(dist),
             stream_ptr(dev.index)))
    return (idx, dist) if return_distance else idx


def knn1(F0, F1, squared=False, return_distance=False):
    return _knn(F0, F1, None, None, None, squared, return_distance)


def knn1_batch(F0, F1, off0, off1, squared=False, return_distance=False):
    """1-NN of every pair (rows off0[p]:off0[p+1] of F0 against rows off1[p]:off1[p+1] of F1) in one library call;
    indices address rows of the concatenated F1."""
    return _knn(F0, F1, off0, off1, None, squared, return_distance)


def knn(F0, F1, k, squared=False, return_distance=False):
    """The k nearest rows of F1 for every row of F0: idx int64 [N0,k] (ascending distance, equal distances by the
    smaller index, column 0 = knn1), dist f32 [N0,k]; columns j >= N1 hold index 0 and distance inf."""
    return _knn(F0, F1, None, None, check_knn_k(k), squared, return_distance)


def knn_batch(F0, F1, off0, off1, k, squared=False, return_distance=False):
    """k-NN of every pair (rows off0[p]:off0[p+1] of F0 against rows off1[p]:off1[p+1] of F1) in one library call:
    idx [off0[-1],k] addresses rows of the concatenated F1 (padding columns of pair p hold off1[p])."""
    return _knn(F0, F1, off0, off1, check_knn_k(k), squared, return_distance)


KNN_TRACE_FIELDS = ('pair', 'table', 'route', 'fallback', 'list_len', 'redo', 'cand_max', 'cand_zero')


def _trace_device(device):
    """The CUDA(ROCm) device of a trace call; ValueError for anything else, before any device state exists."""
    if isinstance(device, (bool, int, float)) or device is None or torch.is_tensor(device):
        raise ValueError(f'expected a device such as "cuda:0", got {device!r}')
    try:
        dev = torch.device(device)
    except (RuntimeError, TypeError) as e:
        raise ValueError(f'expected a device such as "cuda:0", got {device!r}') from e
    if dev.type != 'cuda':
        raise ValueError(f'the k-NN trace lives on a GPU context, got device {dev}')
    return dev


def knn_trace(device, enable):
    """Switch the route trace of the k-NN searches of this thread's context (dgr_ctx_set_knn_trace): a test instrument.
    Off (the default) a search issues exactly the launches it always did; on, every prefiltered table waits for its
    stream and is reduced on the host."""
    dev = _trace_device(device)
    check(_lib.load().dgr_ctx_set_knn_trace(get_ctx(dev), int(bool(enable))))


def knn_trace_rows(device):
    """int32 [npairs, 8] (numpy): one row per pair of the last traced k-NN call on this thread's context, columns
    KNN_TRACE_FIELDS (dgr_debug_knn_trace)."""
    dev = _trace_device(device)
    lib = _lib.load()
    n = C.c_int64(0)
    check(lib.dgr_debug_knn_trace(get_ctx(dev), None, 0, C.byref(n)))
    rows = np.zeros((n.value, len(KNN_TRACE_FIELDS)), np.int32)
    if n.value:
        check(lib.dgr_debug_knn_trace(get_ctx(dev), _np_ptr(rows), n.value, C.byref(n)))
    return rows


def inlier_inputs(coords0, xyz0, coords1, xyz1, idx1, feature_type='coords'):
    lib = _lib.load()
    dev = _dev(xyz0)
    ft = {'ones': 0, 'coords': 1}.get(feature_type)
    if ft is None:
        raise TypeError('Undefined feature type')
    coords0, coords1 = _as(coords0, torch.int32, dev), _as(coords1, torch.int32, dev)
    xyz0, xyz1 = _as(xyz0, torch.float32, dev), _as(xyz1, torch.float32, dev)
    idx1 = _as(idx1, torch.int64, dev).reshape(-1)
    N0 = coords0.shape[0]
    if idx1.shape[0] != N0:
        raise ValueError('one correspondence per row of fragment 0 expected')
    coords6 = torch.empty((N0, 7), dtype=torch.int32, device=dev)
    feats = torch.empty((N0, 6 if ft == 1 else 1), dtype=torch.float32, device=dev)
    check(lib.dgr_inlier_inputs(get_ctx(dev), ptr(coords0), ptr(xyz0), N0, ptr(coords1), ptr(xyz1),
                                coords1.shape[0], ptr(idx1), ft, ptr(coords6), ptr(feats),
                                stream_ptr(dev.index)))
    return coords6, feats


def sigmoid_clip_sum(logit, clip):
    lib = _lib.load()
    dev = _dev(logit)
    logit = _as(logit, torch.float32, dev).reshape(-1)
    w = torch.empty_like(logit)
    s = C.c_double(0)
    check(lib.dgr_sigmoid_clip_sum(get_ctx(dev), ptr(logit), logit.shape[0], float(clip), ptr(w), C.byref(s),
                                   stream_ptr(dev.index)))
    return w.reshape(-1, 1), s.value


def gather_rows3(src, idx):
    lib = _lib.load()
    dev = _dev(src)
    src = _as(src, torch.float32, dev)
    idx = _as(idx, torch.int64, dev).reshape(-1)
    out = torch.empty((idx.shape[0], 3), dtype=torch.float32, device=dev)
    check(lib.dgr_gather_rows3(get_ctx(dev), ptr(src), ptr(idx), idx.shape[0], ptr(out), stream_ptr(dev.index)))
    return out


def _xyw(X, Y, w):
    dev = _dev(X)
    X, Y = _as(X, torch.float32, dev), _as(Y, torch.float32, dev)
    w = _as(w, torch.float32, dev).reshape(-1)
    if X.shape != Y.shape or X.dim() != 2 or X.shape[1] != 3 or w.shape[0] != X.shape[0]:
        raise ValueError('X, Y must be [N,3] and w [N] / [N,1]')
    return dev, X, Y, w


def weighted_procrustes(X, Y, w, eps=F32_EPS):
    lib = _lib.load()
    dev, X, Y, w = _xyw(X, Y, w)
    R = (C.c_float * 9)()
    t = (C.c_float * 3)()
    check(lib.dgr_weighted_procrustes(get_ctx(dev), ptr(X), ptr(Y), ptr(w), X.shape[0], float(eps), R, t,
                                      stream_ptr(dev.index)))
    return np.array(R, np.float32).reshape(3, 3), np.array(t, np.float32)


def se3_refine(X, Y, w, quantization_size=1.0, max_iter=1000, max_break_count=20,
               break_threshold_ratio=1e-5):
    lib = _lib.load()
    dev, X, Y, w = _xyw(X, Y, w)
    R = (C.c_float * 9)()
    t = (C.c_float * 3)()
    it, bc, loss = C.c_int32(0), C.c_int32(0), C.c_float(0)
    check(lib.dgr_se3_refine(get_ctx(dev), ptr(X), ptr(Y), ptr(w), X.shape[0], float(quantization_size),
                             int(max_iter), int(max_break_count), float(break_threshold_ratio), R, t,
                             C.byref(it), C.byref(loss), C.byref(bc), stream_ptr(dev.index)))
    return (np.array(R, np.float32).reshape(3, 3), np.array(t, np.float32),
            {'iterations': it.value, 'loss': loss.value, 'break_count': bc.value})


def se3_refine_from(X, Y, w, state, max_iter, quantization_size=1.0, max_break_count=10 ** 9,
                    break_threshold_ratio=1e-5):
    """Parity instrumentation (dgr_debug_se3_refine_from): the refinement loop resumed at iteration state['i'] from the
    optimiser state `state` = {'i', 'prm' [9], 'm' [9], 'v' [9], 'loss_prev', 'breaks'} (the layout of
    `oracle.registration.global_registration(states=...)`) and run up to iteration `max_iter`.  Returns the end state."""
    lib = _lib.load()
    dev, X, Y, w = _xyw(X, Y, w)
    si = (C.c_double * 30)(*([float(v) for v in state['prm']] + [float(v) for v in state['m']] + [float(v) for v in state['v']]
                             + [float(state['i']), float(state['loss_prev']), float(state['breaks'])]))
    so = (C.c_double * 30)()
    check(lib.dgr_debug_se3_refine_from(get_ctx(dev), ptr(X), ptr(Y), ptr(w), X.shape[0], float(quantization_size),
                                        int(max_iter), int(max_break_count), float(break_threshold_ratio), si, so,
                                        stream_ptr(dev.index)))
    so = np.array(so, np.float64)
    return {'prm': so[:9].copy(), 'm': so[9:18].copy(), 'v': so[18:27].copy(), 'i': int(so[27]), 'loss_prev': float(so[28]),
            'breaks': int(so[29])}


def _xyz_dev(a, dev=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    if dev is None:
        dev = t.device if t.is_cuda else torch.device('cuda', torch.cuda.current_device())
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'expected [N,3] points, got {tuple(t.shape)}')
    return t


def _xyz_any_dev(a):
    """[N,3] float32 / float64 points on the current device in their own dtype."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t if t.is_cuda else t.to(torch.device('cuda', torch.cuda.current_device()))


def icp_point_to_point(source, target, max_correspondence_distance, init=None, max_iter=30,
                       relative_fitness=1e-6, relative_rmse=1e-6):
    """Point-to-point ICP (dgr_icp_point_to_point).  Returns (T [4,4] float64, fitness, inlier_rmse,
    iterations)."""
    lib = _lib.load()
    src = _xyz_dev(source)
    dst = _xyz_dev(target, src.device)
    Ti = None
    if init is not None:
        init = np.ascontiguousarray(np.asarray(init, np.float64))
        if init.shape != (4, 4):
            raise ValueError('init must be a 4x4 matrix')
        Ti = (C.c_double * 16)(*init.reshape(-1))
    T = (C.c_double * 16)()
    st = (C.c_double * 3)()
    check(lib.dgr_icp_point_to_point(get_ctx(src.device), ptr(src), src.shape[0], ptr(dst), dst.shape[0],
                                     float(max_correspondence_distance), Ti, int(max_iter), float(relative_fitness),
                                     float(relative_rmse), T, st, stream_ptr(src.device.index)))
    return np.array(T, np.float64).reshape(4, 4), float(st[0]), float(st[1]), int(st[2])


def ransac_correspondence(X, Y, distance_threshold, num_hypotheses, seed=0):
    """RANSAC over corresponding points X[i] <-> Y[i] (dgr_ransac_correspondence).  Returns
    (T [4,4] float64, best hypothesis index, inlier count, inlier rmse)."""
    lib = _lib.load()
    X = _xyz_dev(X)
    Y = _xyz_dev(Y, X.device)
    if X.shape != Y.shape:
        raise ValueError('X and Y must have the same shape')
    T = (C.c_double * 16)()
    st = (C.c_double * 3)()
    check(lib.dgr_ransac_correspondence(get_ctx(X.device), ptr(X), ptr(Y), X.shape[0], float(distance_threshold),
                                        int(num_hypotheses), int(seed) & 0xffffffff, T, st, stream_ptr(X.device.index)))
    return np.array(T, np.float64).reshape(4, 4), int(st[0]), int(st[1]), float(st[2])


# ----------------------------------------------------------------------------
# ground-truth matches and validation counts (csrc/gtmatch.hip).  Every argument check below runs on the host values
# alone, BEFORE a tensor is moved or the library context is created.
def check_radius_args(radius, K, T, npairs):
    """(radius, K as the C ABI wants it, T float64 [npairs,16]); ValueError for a radius that is not a positive finite
    number, a K that is neither None nor an integer >= 1 (the reference slices idx[:K]), a T that is not [npairs,4,4]
    (or one [4,4] for one pair) of finite numbers."""
    radius = _args.positive_number(radius, 'radius')
    K = 0 if K is None else _args.integer(K, 'K', lambda v: 1 <= v <= np.iinfo(np.int32).max, 'None or an integer >= 1')
    return radius, K, _args.pose_stack(T, npairs, 'T', 4)


def radius_pairs_batch(xyz0, off0, xyz1, off1, T, radius, K=None):
    """Ground-truth correspondences of every pair of a batch (dgr_radius_pairs_batch): pair p = rows off0[p]:off0[p+1] of
    xyz0 under the pose T[p] against rows off1[p]:off1[p+1] of xyz1.  Returns (pairs int64 [P,2] on the device: pair-local
    (i, j) with |T x0[i] - x1[j]| < radius, by i and then by (distance, j), the first K of every i; pair_off int64 numpy
    [npairs+1]: pair p owns pairs[pair_off[p]:pair_off[p+1]])."""
    n0, n1 = _args.rows(xyz0, 3, 'xyz0'), _args.rows(xyz1, 3, 'xyz1')
    o0, o1 = _args.pair_offsets(off0, 'off0', n0), _args.pair_offsets(off1, 'off1', n1)
    if len(o0) != len(o1):
        raise ValueError('off0 and off1 must describe the same number of pairs')
    npairs = len(o0) - 1
    radius, K, T = check_radius_args(radius, K, T, npairs)
    lib = _lib.load()
    xyz0 = _xyz_dev(xyz0)
    dev = xyz0.device
    xyz1 = _xyz_dev(xyz1, dev)
    counts = torch.empty(n0, dtype=torch.int32, device=dev)
    total = C.c_int64(0)

    def call(pairs, capacity):
        check(lib.dgr_radius_pairs_batch(get_ctx(dev), ptr(xyz0), _np_ptr(o0), ptr(xyz1), _np_ptr(o1), npairs, _np_ptr(T),
                                         radius, K, ptr(counts), ptr(pairs), capacity, C.byref(total), stream_ptr(dev.index)))
    call(None, 0)
    pairs = torch.empty((total.value, 2), dtype=torch.int64, device=dev)
    if total.value:
        call(pairs, total.value)
    # pairs of every batch entry: the row counts summed over the entry's rows (bookkeeping on npairs + 1 numbers)
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0, dtype=torch.int64)])
    pair_off = csum[torch.from_numpy(o0).to(dev)].cpu().numpy()
    return pairs, pair_off


def radius_pairs(xyz0, xyz1, T, radius, K=None):
    """One pair: int64 [P,2] (i, j) with |T x0[i] - x1[j]| < radius, the reference's get_matching_indices order."""
    return radius_pairs_batch(xyz0, [0, _args.rows(xyz0, 3, 'xyz0')], xyz1, [0, _args.rows(xyz1, 3, 'xyz1')], T, radius, K)[0]


def pairs_isin(pos, pos_off, pred, pred_off, M):
    """Correctness label of every predicted pair (dgr_pairs_isin_batch): uint8 [Q] on the device, 1 where
    pred[:,0] + pred[:,1] * M[p] occurs among pos[:,0] + pos[:,1] * M[p] of the same batch entry p (wrapping int64).
    pos int64 [P,2], pred int64 [Q,2], pos_off / pred_off [npairs+1], M one integer per batch entry."""
    P, Q = _args.rows(pos, 2, 'pos'), _args.rows(pred, 2, 'pred')
    po, qo = _args.pair_offsets(pos_off, 'pos_off', P), _args.pair_offsets(pred_off, 'pred_off', Q)
    Ms = np.ascontiguousarray(np.asarray(M), dtype=np.int64).reshape(-1)
    if len(po) != len(qo) or len(Ms) != len(po) - 1:
        raise ValueError('pos_off, pred_off and M must describe the same number of pairs')
    lib = _lib.load()
    dev = _dev(pred)
    pos, pred = _as(pos, torch.int64, dev), _as(pred, torch.int64, dev)
    out = torch.empty(Q, dtype=torch.uint8, device=dev)
    check(lib.dgr_pairs_isin_batch(get_ctx(dev), ptr(pos), _np_ptr(po), ptr(pred), _np_ptr(qo), len(Ms), _np_ptr(Ms), ptr(out),
                                   stream_ptr(dev.index)))
    return out


def validation_counts(label, weights, off, threshold=0.5):
    """Per batch entry (n, hits, tp, fp, tn, fn) as int64 numpy [npairs,6] (dgr_validation_counts): label uint8 / bool [Q],
    weights f32 [Q], prediction = weight > threshold."""
    Q = int(label.shape[0]) if hasattr(label, 'shape') and len(label.shape) >= 1 else -1
    if Q < 0 or int(np.prod(tuple(label.shape))) != Q or int(np.prod(tuple(weights.shape))) != Q:
        raise ValueError('label and weights must hold one entry per predicted pair')
    o = _args.pair_offsets(off, 'off', Q)
    if not _args.is_number(threshold) or np.isnan(threshold):   # (any number, +-inf too: not _args.positive_number)
        raise ValueError(f'threshold must be a number, got {threshold!r}')
    lib = _lib.load()
    dev = _dev(weights)
    label = _as(label, torch.uint8, dev).reshape(-1)
    weights = _as(weights, torch.float32, dev).reshape(-1)
    out = np.zeros((len(o) - 1, 6), np.int64)
    check(lib.dgr_validation_counts(get_ctx(dev), ptr(label), ptr(weights), float(threshold), _np_ptr(o), len(o) - 1,
                                    _np_ptr(out), stream_ptr(dev.index)))
    return out


# ----------------------------------------------------------------------------
# geometric fit of registered pairs (csrc/pairscore.hip)
SCORE_WIDTH = 11   # DGR_SCORE_WIDTH: n, sum d^2, sum q (3), sum q q^T upper triangle (6)


def check_score_args(n_rows, bank_off, pair_ids, T, radius):
    """The host-side arguments of `score_pairs` as the C ABI wants them: (off int64 [nfrag+1], ids int32 [n,2],
    T float64 [n,16], radius float).  ValueError for offsets that are not [nfrag+1] integers ascending strictly from >= 0
    to the bank's `n_rows`, a pair list that is empty, not [n,2] integers or names a fragment outside the bank, a T that is
    not [n,4,4] (or one [4,4] for one pair) or has a non-finite entry in its first three rows, a radius that is not a
    positive finite number.  Pure host arithmetic: nothing touches the device."""
    off = _args.fragment_offsets(bank_off, n_rows, 'bank_off')
    ids = _args.pair_ids(pair_ids, len(off) - 1, 'pair_ids')
    radius = _args.positive_number(radius, 'radius')
    return off, ids, _args.pose_stack(T, len(ids), 'T', 3), radius


def score_pairs(bank_xyz, bank_off, pair_ids, T, radius):
    """Sums of every DIRECTED pair (source fragment, target fragment) of a bank under its pose T[k] (source into the
    target's frame), over the source rows that have a target row STRICTLY within `radius` (dgr_score_pairs): float64 numpy
    [n,11] = (n, sum d^2, sum q [3], sum qx qx, qx qy, qx qz, qy qy, qy qz, qz qz) with q the nearest such target row
    (ties: the smaller row).  bank_xyz [N,3] with fragment f in rows bank_off[f]:bank_off[f+1].
    `core.pair_score.scores_from_sums` turns the rows into fitness, inlier RMSE and the 6x6 information matrix."""
    off, ids, T, radius = check_score_args(_args.rows(bank_xyz, 3, 'bank_xyz'), bank_off, pair_ids, T, radius)
    lib = _lib.load()
    xyz = _xyz_dev(bank_xyz)
    dev = xyz.device
    out = np.zeros((len(ids), SCORE_WIDTH), np.float64)
    check(lib.dgr_score_pairs(get_ctx(dev), ptr(xyz), _np_ptr(off), len(off) - 1, _np_ptr(ids), len(ids), _np_ptr(T), radius,
                              _np_ptr(out), stream_ptr(dev.index)))
    return out


# ----------------------------------------------------------------------------
# averaging voxel down-sample / scene fusion (csrc/voxelmean.hip)
VM_FRAC_BITS = 40   # DGR_VM_FRAC_BITS: a voxel's sums count 2^-40 of a voxel


def check_voxel_mean_args(xyz, voxel_size, off=None, frag_ids=None, T=None, origin=None):
    """The host-side arguments of `voxel_mean` as the C ABI wants them: (off int64 [nfrag+1], ids int32 [nsel] or None,
    T float64 [nsel,16] or None, origin float64 [3], voxel_size float, selected rows).  ValueError for an `xyz` that is not
    a float32 / float64 [N,3] array or tensor, a voxel size that is not a positive finite number, offsets that are not
    [nfrag+1] integers ascending strictly from >= 0 to the row count, a fragment list that is empty, not 1-D integers
    (or a bool mask over the fragments), repeats a fragment or names one outside the bank, a T that is not [nsel,4,4]
    (or one [4,4] for one fragment) or has a non-finite entry in its first three rows, an origin that is not three finite
    numbers, 2^31 or more selected rows.  Pure host arithmetic: nothing touches the device."""
    if not (torch.is_tensor(xyz) or isinstance(xyz, np.ndarray)):
        raise ValueError('xyz must be a numpy array or a torch tensor')
    if str(xyz.dtype).replace('torch.', '') not in ('float32', 'float64'):
        raise ValueError(f'xyz must be float32 or float64, got {xyz.dtype}')
    return check_voxel_mean_rows(_args.rows(xyz, 3, 'xyz'), voxel_size, off, frag_ids, T, origin)


def check_voxel_mean_rows(n_rows, voxel_size, off=None, frag_ids=None, T=None, origin=None):
    """`check_voxel_mean_args` behind the check of `xyz` itself, for a point array of `n_rows` rows."""
    voxel_size = _args.positive_number(voxel_size, 'voxel_size')
    if off is None:
        if n_rows == 0:
            raise ValueError('empty point cloud')
        off = np.array([0, n_rows], np.int64)
    else:
        off = _args.fragment_offsets(off, n_rows, 'off')
    nfrag = len(off) - 1
    ids = None
    if frag_ids is not None:
        ids = np.asarray(frag_ids.cpu() if torch.is_tensor(frag_ids) else frag_ids)
        if ids.dtype == np.bool_:
            if ids.shape != (nfrag,):
                raise ValueError(f'a fragment mask must be [{nfrag}], got {ids.shape}')
            ids = np.nonzero(ids)[0]
        if ids.size == 0:
            raise ValueError('the fragment list is empty')
        if ids.ndim != 1 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError('frag_ids must be a 1-D integer array or a bool mask over the fragments')
        if bool((ids < 0).any()) or bool((ids >= nfrag).any()):
            raise ValueError(f'fragment id outside [0, {nfrag})')
        if len(np.unique(ids)) != len(ids):
            raise ValueError('a fragment id is repeated')
        ids = np.ascontiguousarray(ids, dtype=np.int32)
    nsel = nfrag if ids is None else len(ids)
    if T is not None:
        T = _args.pose_stack(T, nsel, 'T', 3)
    try:
        origin = np.zeros(3) if origin is None else np.ascontiguousarray(_args.host(origin), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('origin must be three finite numbers') from None
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError('origin must be three finite numbers')
    rows = int(np.diff(off).sum() if ids is None else (off[ids.astype(np.int64) + 1] - off[ids]).sum())
    if rows >= 2 ** 31:
        raise ValueError(f'{rows} selected rows: 2^31 or more')
    return off, ids, T, origin, voxel_size, rows


def voxel_mean(xyz, voxel_size, off=None, frag_ids=None, T=None, origin=None, return_sums=False):
    """Averaging voxel down-sample (dgr_voxel_mean): every occupied voxel of the lattice (`origin`, default 0; `voxel_size`)
    is replaced by the mean of the points in it.  xyz [N,3] float32 or float64 (quantised in its own dtype widened exactly),
    fragment f in rows off[f]:off[f+1] (default: one fragment); `frag_ids`: the distinct fragments that take part (ids or a
    bool mask; default all), T[k] [4,4] the pose of fragment frag_ids[k] into the common frame (default: no transform).
    Returns a dict of device tensors in ascending order of a voxel's first row of `xyz`: `xyz` float64 [V,3] the means,
    `coords` int32 [V,3], `count` int32 [V], `first` int64 [V], with `sums` int64 [V,3] when `return_sums` (the fixed-point
    sums, VM_FRAC_BITS fractional bits: what is bitwise comparable), and `dropped` (int): rows that are not finite or fall
    outside the int32 lattice.  Integer accumulation: two runs agree bit for bit, whatever the order of the rows."""
    off, ids, T, origin, voxel_size, rows = check_voxel_mean_args(xyz, voxel_size, off, frag_ids, T, origin)
    lib = _lib.load()
    t = _xyz_any_dev(xyz).contiguous()
    dev = t.device
    first = torch.empty(rows, dtype=torch.int64, device=dev)
    coords = torch.empty((rows, 3), dtype=torch.int32, device=dev)
    count = torch.empty(rows, dtype=torch.int32, device=dev)
    sums = torch.empty((rows, 3), dtype=torch.int64, device=dev) if return_sums else None
    mean = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    n, dropped = C.c_int64(0), C.c_int64(0)
    check(lib.dgr_voxel_mean(get_ctx(dev), ptr(t), int(t.dtype == torch.float64), _np_ptr(off), len(off) - 1,
                             _np_ptr(ids), len(off) - 1 if ids is None else len(ids), _np_ptr(T), _np_ptr(origin),
                             voxel_size, ptr(first), ptr(coords), ptr(count), ptr(sums), ptr(mean), C.byref(n),
                             C.byref(dropped), stream_ptr(dev.index)))
    V = n.value
    out = {'xyz': mean[:V], 'coords': coords[:V], 'count': count[:V], 'first': first[:V], 'dropped': int(dropped.value)}
    if return_sums:
        out['sums'] = sums[:V]
    return out


# ----------------------------------------------------------------------------
# TSDF fusion of depth frames into a fragment (csrc/tsdf.hip)
TSDF_BLOCK_LIMIT = 2 ** 26   # DGR_TSDF_BLOCK_LIMIT
TSDF_FIRST_POINTS, TSDF_FIRST_BLOCKS = 1 << 20, 1 << 10   # tsdf_fragment's first output arrays; it asks again when they are small


def check_tsdf_args(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale=1000.0, depth_trunc=4.5, block=16, stride=4,
                    min_weight=1):
    """The host-side arguments of `tsdf_fragment` as the C ABI wants them: (intrinsic float64 [4], pose float64 [F,16],
    extrinsic float64 [F,16] = inv(pose), (F, H, W)).  ValueError for a `depth` that is not a uint16 [F,H,W] array or tensor
    with F, H, W >= 1, intrinsics that are not four finite numbers with fx, fy > 0, poses that are not [F,4,4] (or one
    [4,4] for one frame), not finite or singular, a `block` other than 8 or 16, a voxel length, depth scale or depth
    truncation that is not a positive finite number, an `sdf_trunc` outside (0, voxel_length * block], `stride` < 1,
    `min_weight` < 1, 2^28 or more strided pixels.  Pure host arithmetic: nothing touches the device."""
    if not (torch.is_tensor(depth) or isinstance(depth, np.ndarray)):
        raise ValueError('depth must be a numpy array or a torch tensor')
    if str(depth.dtype).replace('torch.', '') != 'uint16':
        raise ValueError(f'depth must be uint16, got {depth.dtype}')
    if depth.ndim != 3 or min(depth.shape) < 1:
        raise ValueError(f'depth must be [F,H,W] with F, H, W >= 1, got {tuple(depth.shape)}')
    F, H, W = (int(v) for v in depth.shape)
    voxel_length = _args.positive_number(voxel_length, 'voxel_length')
    sdf_trunc = _args.positive_number(sdf_trunc, 'sdf_trunc')
    depth_scale = _args.positive_number(depth_scale, 'depth_scale')
    depth_trunc = _args.positive_number(depth_trunc, 'depth_trunc')
    block = _args.integer(block, 'block', lambda v: v in (8, 16), '8 or 16')
    stride = _args.integer(stride, 'stride', lambda v: v >= 1, 'an integer >= 1')
    min_weight = _args.integer(min_weight, 'min_weight', lambda v: 1 <= v < 2 ** 31, 'an integer >= 1')
    if sdf_trunc > voxel_length * block:
        raise ValueError(f'sdf_trunc {sdf_trunc} exceeds a block ({voxel_length} x {block}): a pixel would touch more than '
                         f'two blocks per axis')
    try:
        intrinsic = np.ascontiguousarray(_args.host(intrinsic), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('intrinsic must be four finite numbers (fx, fy, cx, cy)') from None
    if intrinsic.shape != (4,) or not np.isfinite(intrinsic).all():
        raise ValueError('intrinsic must be four finite numbers (fx, fy, cx, cy)')
    if intrinsic[0] <= 0 or intrinsic[1] <= 0:
        raise ValueError('fx and fy must be positive')
    # (not _args.pose_stack: a pose is inverted below, so its dtype is checked too and it stays [F,4,4])
    pose = _args.host(pose)
    if pose.shape == (4, 4) and F == 1:
        pose = pose[None]
    if pose.shape != (F, 4, 4) or pose.dtype.kind not in 'fiu':
        raise ValueError(f'pose must be [{F},4,4], got {pose.shape}')
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    if not np.isfinite(pose).all():
        raise ValueError('pose must be finite')
    try:
        extrinsic = np.ascontiguousarray(np.linalg.inv(pose))
    except np.linalg.LinAlgError:
        raise ValueError('a pose is singular') from None
    if not np.isfinite(extrinsic).all():
        raise ValueError('a pose is singular')
    if F * (-(-H // stride)) * (-(-W // stride)) >= 2 ** 28:
        raise ValueError('2^28 or more strided pixels: raise the stride')
    return intrinsic, pose.reshape(F, 16), extrinsic.reshape(F, 16), (F, H, W)


TSDF_COLOR_MAX_FRAMES = 8421504   # DGR_TSDF_COLOR_MAX_FRAMES: 255 F fits an int32


def check_tsdf_color_args(color, depth):
    """The `color` argument of `tsdf_fragment` against its (already checked) `depth`.  ValueError for a `color` that is not
    uint8, not `depth`'s [F,H,W] with a last axis of 3, a tensor on another device than a `depth` that is a tensor, more than
    TSDF_COLOR_MAX_FRAMES frames (a voxel's colour sum could pass 2^31).  Only `dtype`, `shape` and (of tensors) `device` are
    looked at: nothing touches the device."""
    if not (hasattr(color, 'dtype') and hasattr(color, 'shape')):
        raise ValueError('color must be a numpy array or a torch tensor')
    if str(color.dtype).replace('torch.', '') != 'uint8':
        raise ValueError(f'color must be uint8, got {color.dtype}')
    want = tuple(int(v) for v in depth.shape) + (3,)
    if tuple(int(v) for v in color.shape) != want:
        raise ValueError(f'color must be [F,H,W,3] = {list(want)} like depth, got {list(color.shape)}')
    if torch.is_tensor(color) and torch.is_tensor(depth) and color.device != depth.device:
        raise ValueError(f'color is on {color.device}, depth on {depth.device}')
    if want[0] > TSDF_COLOR_MAX_FRAMES:
        raise ValueError(f'{want[0]} frames with colour: at most {TSDF_COLOR_MAX_FRAMES} (255 F must fit an int32)')


def tsdf_fragment(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale=1000.0, depth_trunc=4.5, block=16, stride=4,
                  min_weight=1, return_volume=False, return_stats=False, color=None):
    """TSDF fusion of F depth frames under their camera poses and the surface points of the fused volume
    (dgr_tsdf_fragment; what the reference's util/integration.py does with Open3D's ScalableTSDFVolume).  depth uint16
    [F,H,W] (numpy or a device tensor), intrinsic = (fx, fy, cx, cy), pose [F,4,4] float64 camera-to-world as the
    `.pose.txt` files give it; `extrinsic = inv(pose)` is taken here, on the host (any finite, invertible pose: it need
    not be rigid).  Blocks of `block`^3 voxels of
    `voxel_length` are allocated where the pixels on a grid of `stride` see a surface, within `sdf_trunc` of it; every
    voxel of these blocks is integrated over all frames in order; the points are the zero crossings on the voxels' +x,
    +y, +z edges whose two ends have at least `min_weight` observations.
    Returns xyz float64 [P,3] on the device; with `return_volume` a dict with `xyz`, `blocks` int32 [nb,3], `tsdf`
    float32 [nb, block^3] and `weight` int32 [nb, block^3]; with `return_stats` the dict also has `kept`, the (block,
    frame) pairs the integration did not cull.  Two calls agree bit for bit.
    `color` uint8 [F,H,W,3] (R, G, B; numpy or a tensor on `depth`'s device) is fused with the depth (dgr_tsdf_fragment_rgb):
    a voxel sums the colour of every pixel that updates it, a point gets the two ends' mean colours blended as its position
    is.  The result is then always a dict: `xyz`, `color` float64 [P,3] in [0, 1], with `return_volume` also `rgb_sum`
    int32 [nb, block^3, 3]; `xyz`, `blocks`, `tsdf` and `weight` are exactly those of the call without `color`."""
    intrinsic, pose, extrinsic, (F, H, W) = check_tsdf_args(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale,
                                                            depth_trunc, block, stride, min_weight)
    if color is not None:
        check_tsdf_color_args(color, depth)
    lib = _lib.load()
    if torch.is_tensor(depth):
        _dev(depth)
        d = depth.contiguous()
    else:
        # torch has no arithmetic on uint16 and older versions no uint16 at all: the bytes travel as int16
        a = np.ascontiguousarray(depth)
        d = torch.from_numpy((a if a.flags.writeable else a.copy()).view(np.int16))
        d = d.to(color.device) if torch.is_tensor(color) and color.is_cuda else d.cuda()
    dev = d.device
    if torch.is_tensor(color):
        _dev(color)
        col = color.contiguous()
    elif color is not None:
        a = np.ascontiguousarray(color)
        col = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    V = block ** 3
    max_points, max_blocks = TSDF_FIRST_POINTS, TSDF_FIRST_BLOCKS
    nb, npts, kept = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    while True:
        xyz = torch.empty((max_points, 3), dtype=torch.float64, device=dev)
        blocks = tsdf = weight = rgb_sum = pcolor = None
        if return_volume:
            blocks = torch.empty((max_blocks, 3), dtype=torch.int32, device=dev)
            tsdf = torch.empty((max_blocks, V), dtype=torch.float32, device=dev)
            weight = torch.empty((max_blocks, V), dtype=torch.int32, device=dev)
        args = (get_ctx(dev), ptr(d), F, H, W, _np_ptr(intrinsic), _np_ptr(pose), _np_ptr(extrinsic), float(voxel_length),
                float(sdf_trunc), float(depth_scale), float(depth_trunc), int(block), int(stride), int(min_weight), ptr(xyz),
                max_points, ptr(blocks), ptr(tsdf), ptr(weight), max_blocks if return_volume else 0, C.byref(nb),
                C.byref(npts), C.byref(kept) if return_stats else None)
        if color is None:
            rc = lib.dgr_tsdf_fragment(*args, stream_ptr(dev.index))
        else:
            pcolor = torch.empty((max_points, 3), dtype=torch.float64, device=dev)
            if return_volume:
                rgb_sum = torch.empty((max_blocks, V, 3), dtype=torch.int32, device=dev)
            rc = lib.dgr_tsdf_fragment_rgb(*args, ptr(col), ptr(rgb_sum), ptr(pcolor), stream_ptr(dev.index))
        # the one recoverable failure: an output array too small for what the call found -- it says how much it needs
        if rc == _lib.DGR_ENOMEM and ((return_volume and nb.value > max_blocks) or npts.value > max_points):
            max_blocks, max_points = max(max_blocks, nb.value), max(max_points, npts.value)
            continue
        check(rc)
        break
    xyz = xyz[:npts.value]
    if not (return_volume or return_stats or color is not None):
        return xyz
    out = {'xyz': xyz}
    if color is not None:
        out['color'] = pcolor[:npts.value]
    if return_volume:
        out.update(blocks=blocks[:nb.value], tsdf=tsdf[:nb.value], weight=weight[:nb.value])
        if color is not None:
            out['rgb_sum'] = rgb_sum[:nb.value]
    if return_stats:
        out.update(kept=int(kept.value), n_blocks=int(nb.value))
    return out


# ----------------------------------------------------------------------------
# triangle mesh and vertex normals of a fused TSDF volume (csrc/tsdfmesh.hip)
TSDF_MESH_FIRST_VERTICES, TSDF_MESH_FIRST_TRIANGLES = 1 << 20, 1 << 21   # tsdf_mesh's first output arrays; it asks again when they are small


def check_tsdf_mesh_color_args(rgb_sum, tsdf):
    """The `rgb_sum` argument of `tsdf_mesh` against its (already checked) `tsdf`: ValueError unless it is an int32 tensor
    [nb, block^3, 3] on `tsdf`'s device.  Nothing touches the device."""
    if not torch.is_tensor(rgb_sum) or rgb_sum.device != tsdf.device:
        raise ValueError("rgb_sum must be a tensor on tsdf's device")
    if rgb_sum.dtype != torch.int32 or tuple(rgb_sum.shape) != tuple(tsdf.shape) + (3,):
        raise ValueError(f'rgb_sum must be int32 {list(tsdf.shape) + [3]}, got {rgb_sum.dtype} {list(rgb_sum.shape)}')


def check_tsdf_mesh_args(blocks, tsdf, weight, voxel_length, block=16, min_weight=1):
    """The arguments of `tsdf_mesh` checked on the host: (nb, voxel_length, block, min_weight).  ValueError for tensors that
    are not on one GPU, a `blocks` that is not int32 [nb,3], a `tsdf` that is not float32 [nb, block^3], a `weight` that is
    not int32 of `tsdf`'s shape, a `block` other than 8 or 16, a `voxel_length` that is not a positive finite number,
    `min_weight` < 1, 5 nb block^3 >= 2^31.  Nothing touches the device (block coordinates are checked there)."""
    voxel_length = _args.positive_number(voxel_length, 'voxel_length')
    block = _args.integer(block, 'block', lambda v: v in (8, 16), '8 or 16')
    min_weight = _args.integer(min_weight, 'min_weight', lambda v: 1 <= v < 2 ** 31, 'an integer >= 1')
    for t, name in ((blocks, 'blocks'), (tsdf, 'tsdf'), (weight, 'weight')):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f'{name} must be a tensor on the GPU')
    if not (blocks.device == tsdf.device == weight.device):
        raise ValueError('blocks, tsdf and weight must be on one device')
    if blocks.dtype != torch.int32 or blocks.ndim != 2 or blocks.shape[1] != 3:
        raise ValueError(f'blocks must be int32 [nb,3], got {blocks.dtype} {tuple(blocks.shape)}')
    nb = int(blocks.shape[0])
    if tsdf.dtype != torch.float32 or tuple(tsdf.shape) != (nb, block ** 3):
        raise ValueError(f'tsdf must be float32 [{nb},{block ** 3}], got {tsdf.dtype} {tuple(tsdf.shape)}')
    if weight.dtype != torch.int32 or tuple(weight.shape) != (nb, block ** 3):
        raise ValueError(f'weight must be int32 [{nb},{block ** 3}], got {weight.dtype} {tuple(weight.shape)}')
    if 5 * nb * block ** 3 >= 2 ** 31:
        raise ValueError(f'{nb} blocks of {block}^3 voxels: 2^31 or more possible triangles')
    return nb, voxel_length, block, min_weight


def tsdf_mesh(blocks, tsdf, weight, voxel_length, block=16, min_weight=1, normals=True, rgb_sum=None):
    """Triangle mesh and vertex normals of a fused TSDF volume (dgr_tsdf_mesh; Open3D's extract_triangle_mesh in the
    reference's util/integration.py).  blocks int32 [nb,3], tsdf float32 [nb, block^3], weight int32 [nb, block^3]: device
    tensors as `tsdf_fragment(..., return_volume=True)` returns them, or a volume made by hand in that layout.
    Returns a dict of device tensors: `xyz` float64 [P,3] -- the very points of `tsdf_fragment`, in its order --, `normal`
    float64 [P,3] (unit, from negative to positive; absent without `normals`) and `triangles` int32 [T,3], wound so that
    they face the positive side.  Two calls agree bit for bit.  With `rgb_sum` int32 [nb, block^3, 3], the colour sums of
    `tsdf_fragment(..., color=..., return_volume=True)`, also `color` float64 [P,3] in [0, 1]: the very colours of that call's
    points (dgr_tsdf_mesh_rgb); the rest of the dict is what it is without `rgb_sum`."""
    nb, voxel_length, block, min_weight = check_tsdf_mesh_args(blocks, tsdf, weight, voxel_length, block, min_weight)
    if rgb_sum is not None:
        check_tsdf_mesh_color_args(rgb_sum, tsdf)
        rgb_sum = rgb_sum.contiguous()
    lib = _lib.load()
    dev = blocks.device
    blocks, tsdf, weight = blocks.contiguous(), tsdf.contiguous(), weight.contiguous()
    max_v, max_t = TSDF_MESH_FIRST_VERTICES, TSDF_MESH_FIRST_TRIANGLES
    nv, nt = C.c_int64(0), C.c_int64(0)
    while True:
        xyz = torch.empty((max_v, 3), dtype=torch.float64, device=dev)
        normal = torch.empty((max_v, 3), dtype=torch.float64, device=dev) if normals else None
        tri = torch.empty((max_t, 3), dtype=torch.int32, device=dev)
        args = (get_ctx(dev), ptr(blocks), nb, ptr(tsdf), ptr(weight), block, voxel_length, min_weight, ptr(xyz), ptr(normal),
                max_v, ptr(tri), max_t, C.byref(nv), C.byref(nt))
        if rgb_sum is None:
            rc = lib.dgr_tsdf_mesh(*args, stream_ptr(dev.index))
        else:
            vcolor = torch.empty((max_v, 3), dtype=torch.float64, device=dev)
            rc = lib.dgr_tsdf_mesh_rgb(*args, ptr(rgb_sum), ptr(vcolor), stream_ptr(dev.index))
        # the one recoverable failure: an output array too small -- the call says how much both need
        if rc == _lib.DGR_ENOMEM and (nv.value > max_v or nt.value > max_t):
            max_v, max_t = max(max_v, nv.value), max(max_t, nt.value)
            continue
        check(rc)
        break
    out = {'xyz': xyz[:nv.value], 'triangles': tri[:nt.value]}
    if normals:
        out['normal'] = normal[:nv.value]
    if rgb_sum is not None:
        out['color'] = vcolor[:nv.value]
    return out


# ----------------------------------------------------------------------------
# pose-graph optimisation over scored pairs (csrc/posegraph.hip)
PG_MAX_NODES = 128   # DGR_PG_MAX_NODES


def check_pose_graph_args(node_off, edge_off, edge_ids, edge_T, edge_info, edge_uncertain, pose_init, params):
    """The arguments of `pose_graph_optimize` as the C ABI wants them: (node_off int64 [g+1], edge_off int64 [g+1],
    ids int32 [E,2], X float64 [E,16], info float64 [E,36], uncertain uint8 [E], poses float64 [N,16], params: one
    (mu, reference_node, max_iter, rel_tol) tuple per graph).  `params` is one such tuple or dict per graph (`max_iter`
    and `rel_tol` may be left out: 100, 1e-13).  ValueError for: offsets that are not integers ascending from 0, an empty
    graph (no nodes or no edges), more than PG_MAX_NODES nodes in a graph, an edge id outside its graph, an edge from a
    node to itself, a non-finite X, information matrix or initial pose, mu <= 0, a reference node outside the graph, a
    negative max_iter or rel_tol, arrays whose shapes do not fit.  Pure host arithmetic: nothing touches the device."""
    offs = []
    for name, o in (('node_off', node_off), ('edge_off', edge_off)):   # (from 0 exactly, and other words than a bank's)
        o = _args.host(o)
        if o.ndim != 1 or len(o) < 2 or not np.issubdtype(o.dtype, np.integer):
            raise ValueError(f'{name} must be a 1-D integer array [ngraphs+1]')
        o = np.ascontiguousarray(o, dtype=np.int64)
        if o[0] != 0 or bool((np.diff(o) < 1).any()):
            raise ValueError(f'{name} must ascend strictly from 0: a graph without nodes or edges is refused')
        offs.append(o)
    noff, eoff = offs
    if len(noff) != len(eoff):
        raise ValueError('node_off and edge_off must have one entry per graph and one more')
    ng, N, E = len(noff) - 1, int(noff[-1]), int(eoff[-1])
    n_of = np.diff(noff)
    if bool((n_of > PG_MAX_NODES).any()):
        raise ValueError(f'a graph has {int(n_of.max())} nodes: at most {PG_MAX_NODES} (6 (n - 1) = 762 unknowns and a '
                         '4.6 MB normal matrix per graph)')
    ids = _args.host(edge_ids)
    if ids.shape != (E, 2) or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f'edge_ids must be an [{E},2] integer array')
    n_edge = np.repeat(n_of, np.diff(eoff))
    if bool((ids < 0).any()) or bool((ids >= n_edge[:, None]).any()):
        raise ValueError('edge id outside its graph')
    if bool((ids[:, 0] == ids[:, 1]).any()):
        raise ValueError('an edge joins a node to itself')
    ids = np.ascontiguousarray(ids, dtype=np.int32)

    def mats(a, k, n, name):   # (not _args.pose_stack: 6x6 too, and one matrix does not stand for a stack of one)
        a = _args.host(a)
        if a.shape != (n, k, k):
            raise ValueError(f'{name} must be [{n},{k},{k}], got {a.shape}')
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(n, k * k)
        if not np.isfinite(a).all():
            raise ValueError(f'{name} must be finite')
        return a
    X, info, poses = mats(edge_T, 4, E, 'edge_T'), mats(edge_info, 6, E, 'edge_info'), mats(pose_init, 4, N, 'pose_init')
    unc = _args.host(edge_uncertain)
    if unc.shape != (E,):
        raise ValueError(f'edge_uncertain must be [{E}]')
    unc = np.ascontiguousarray(unc.astype(bool), dtype=np.uint8)
    if isinstance(params, dict) or (isinstance(params, tuple) and not isinstance(params[0], (tuple, list, dict))):
        params = [params]
    if len(params) != ng:
        raise ValueError('one parameter record per graph expected')
    out = []
    for g, p in enumerate(params):
        if isinstance(p, dict):
            p = (p['mu'], p.get('reference_node', 0), p.get('max_iter', 100), p.get('rel_tol', 1e-13))
        p = tuple(p) + (0, 100, 1e-13)[len(p) - 1:]
        mu, ref, max_iter, rel_tol = float(p[0]), int(p[1]), int(p[2]), float(p[3])
        if not (mu > 0 and np.isfinite(mu)):
            raise ValueError(f'graph {g}: mu must be positive and finite, got {mu!r}')
        if not 0 <= ref < n_of[g]:
            raise ValueError(f'graph {g}: reference node {ref} outside [0, {int(n_of[g])})')
        if not 0 <= max_iter <= 100000:
            raise ValueError(f'graph {g}: max_iter = {max_iter}')
        if not (rel_tol >= 0 and np.isfinite(rel_tol)):
            raise ValueError(f'graph {g}: rel_tol must be >= 0 and finite')
        out.append((mu, ref, max_iter, rel_tol))
    return noff, eoff, ids, X, info, unc, poses, out


def pose_graph_optimize(node_off, edge_off, edge_ids, edge_T, edge_info, edge_uncertain, pose_init, params, device='cuda'):
    """Robust pose-graph optimisation with line processes of `ngraphs` independent graphs in one library call
    (dgr_pose_graph_optimize; one workgroup per graph): graph g owns nodes node_off[g]:node_off[g+1] and edges
    edge_off[g]:edge_off[g+1]; edge_ids [E,2] = (s, t) LOCAL to the graph, edge_T [E,4,4] the pose of s in t's frame,
    edge_info [E,6,6], edge_uncertain [E], pose_init [N,4,4], params as for `check_pose_graph_args`.  Host arrays in,
    host arrays out: (poses [N,4,4], line_process [E], stats [ngraphs,4] = F* initial, F* final, accepted steps,
    converged).  `core.pose_graph` states the objective; the reference node of every graph keeps its pose bit for bit."""
    noff, eoff, ids, X, info, unc, poses, prm = check_pose_graph_args(node_off, edge_off, edge_ids, edge_T, edge_info,
                                                                      edge_uncertain, pose_init, params)
    lib = _lib.load()
    dev = torch.device(device)
    ng = len(noff) - 1
    cp = (_lib.PgParams * ng)(*[_lib.PgParams(*p) for p in prm])
    pose_out, line, stats = np.zeros_like(poses), np.zeros(len(ids)), np.zeros((ng, 4))
    with torch.cuda.device(dev):
        check(lib.dgr_pose_graph_optimize(get_ctx(dev), ng, _np_ptr(noff), _np_ptr(eoff), _np_ptr(ids), _np_ptr(X),
                                          _np_ptr(info), _np_ptr(unc), _np_ptr(poses), cp, _np_ptr(pose_out), _np_ptr(line),
                                          _np_ptr(stats), stream_ptr(dev.index)))
    return pose_out.reshape(-1, 4, 4), line, stats


# ----------------------------------------------------------------------------
# what the two entry points of the fused pipeline share: the parameter record, the two test hooks, the outputs
def _register_params(voxel_size, clip_weight_thresh, inlier_feature_type, max_iter, max_break_count, break_threshold_ratio,
                     skip_refinement, safeguard, use_icp, ransac_hypotheses, ransac_seed):
    return _lib.Params(float(clip_weight_thresh), float(voxel_size),
                       {'ones': 0, 'coords': 1}[inlier_feature_type], int(max_iter), int(max_break_count),
                       float(break_threshold_ratio), int(bool(skip_refinement)), int(bool(safeguard)),
                       int(ransac_hypotheses), int(ransac_seed) & 0xffffffff, int(bool(use_icp)))


def _register_out(npairs):
    """(T float32 [npairs,16] -- float64 comes through `_register_T64` --, status int32 [npairs], stats float32 [npairs,4])"""
    return np.empty((npairs, 16), np.float32), np.empty(npairs, np.int32), np.empty((npairs, 4), np.float32)


def _register_hooks(forced_logit, override_idx1, n0, dev):
    """(forced_logit f32, override_idx1 int64), each flat on `dev` or None; one given must hold `n0` entries, the rows of
    the batch's concatenated fragment 0 (n0 None: the count is not known and not checked)."""
    out = []
    for t, dtype, name in ((forced_logit, torch.float32, 'forced_logit'), (override_idx1, torch.int64, 'override_idx1')):
        if t is not None:
            t = _as(t, dtype, dev).reshape(-1)
            if n0 is not None and t.shape[0] != n0:
                raise ValueError(f'{name} must have one entry per row of fragment 0')
        out.append(t)
    return out


def _register_T64(lib, dev, npairs):
    """T float64 [npairs,4,4] of the call that just returned: always at full width, whatever the flags (the RANSAC / ICP
    stages compute in float64 like Open3D; without them the f32 estimate widens exactly): one return dtype.  The library
    clears its float64 copy when a call starts, so a call that failed midway cannot leave an earlier batch's transforms
    to be read here."""
    T64 = np.empty((npairs, 16), np.float64)
    n = C.c_int64(0)
    check(lib.dgr_register_batch_f64(get_ctx(dev), _np_ptr(T64), npairs, C.byref(n)))
    if n.value != npairs:
        raise RuntimeError(f'dgr_register_batch_f64 holds {n.value} pairs, expected {npairs}')
    return T64.reshape(npairs, 4, 4)


def register_batch(fcgf, inlier, coords0, xyz0, off0, coords1, xyz1, off1, voxel_size,
                   clip_weight_thresh=0.05, inlier_feature_type='coords', max_iter=1000,
                   max_break_count=20, break_threshold_ratio=1e-4, skip_refinement=False,
                   forced_logit=None, override_idx1=None, safeguard=False, use_icp=False, ransac_hypotheses=4000000,
                   ransac_seed=0):
    """Fused pipeline over a batch of voxelised pairs (dgr_register_batch).  Returns
    T [npairs,4,4] float64 (what the reference's register() returns; fetched through dgr_register_batch_f64: the learned
    f32 estimate widens exactly, the safeguard / ICP stages compute in float64), status [npairs] int32, stats [npairs,4] float32.
    `status` is a CODE plus FLAG bits:
    `status & _lib.STATUS_MASK` is 0 ok / 1 low confidence / 2 SVD failed / 3 safeguard (T from the RANSAC), and
    `_lib.STATUS_FLAG_ICP_SKIPPED` (0x100) is OR-ed on when `use_icp` was asked for but the final ICP could not run on the
    pair -- compare the masked code, not the raw word."""
    lib = _lib.load()
    dev = fcgf.device
    npairs = len(off0) - 1
    coords0, coords1 = _as(coords0, torch.int32, dev), _as(coords1, torch.int32, dev)
    xyz0, xyz1 = _as(xyz0, torch.float32, dev), _as(xyz1, torch.float32, dev)
    o0 = (C.c_int64 * (npairs + 1))(*[int(v) for v in off0])
    o1 = (C.c_int64 * (npairs + 1))(*[int(v) for v in off1])
    if coords0.shape[0] != off0[-1] or coords1.shape[0] != off1[-1]:
        raise ValueError('offset arrays do not match the coordinate arrays')
    prm = _register_params(voxel_size, clip_weight_thresh, inlier_feature_type, max_iter, max_break_count,
                           break_threshold_ratio, skip_refinement, safeguard, use_icp, ransac_hypotheses, ransac_seed)
    T, status, stats = _register_out(npairs)
    fl, ov = _register_hooks(forced_logit, override_idx1, coords0.shape[0], dev)
    check(lib.dgr_register_batch(get_ctx(dev), fcgf.handle, inlier.handle, ptr(coords0), ptr(xyz0), o0,
                                 ptr(coords1), ptr(xyz1), o1, npairs, C.byref(prm), ptr(ov), ptr(fl),
                                 _np_ptr(T), _np_ptr(status), _np_ptr(stats), stream_ptr(dev.index)))
    return _register_T64(lib, dev, npairs), status, stats


def register_pairs(inlier, bank_coords, bank_xyz, bank_F, bank_off, pair_ids, voxel_size,
                   clip_weight_thresh=0.05, inlier_feature_type='coords', max_iter=1000,
                   max_break_count=20, break_threshold_ratio=1e-4, skip_refinement=False,
                   forced_logit=None, override_idx1=None, safeguard=False, use_icp=False, ransac_hypotheses=4000000,
                   ransac_seed=0):
    """`register_batch` for pairs of fragments whose FCGF features exist already (dgr_register_pairs): the bank is
    coords int32 [N,4], xyz f32 [N,3], F f32 [N,C] on the device of `inlier` with fragment f in rows
    bank_off[f]:bank_off[f+1] (host, [nfrag+1]); pair_ids is [npairs,2] (fragment 0, fragment 1).  The library copies the
    rows into the batch layout and runs the stages behind the FCGF net; `forced_logit` (one value per row of the pairs'
    concatenated fragment 0) and `override_idx1` (rows of the concatenated fragment 1) mean what they mean there.
    Returns T [npairs,4,4] float64, status [npairs] int32, stats [npairs,4] float32, as `register_batch` does."""
    lib = _lib.load()
    dev = inlier.device
    off = np.ascontiguousarray(np.asarray(bank_off), dtype=np.int64).reshape(-1)
    ids = np.ascontiguousarray(np.asarray(pair_ids), dtype=np.int32)
    if ids.ndim != 2 or ids.shape[1] != 2:
        raise ValueError('pair_ids must be [npairs,2]')
    npairs, nfrag = len(ids), len(off) - 1
    bank_coords, bank_xyz = _as(bank_coords, torch.int32, dev), _as(bank_xyz, torch.float32, dev)
    bank_F = _as(bank_F, torch.float32, dev)
    if nfrag < 1 or bank_coords.shape[0] != off[-1] or bank_xyz.shape[0] != off[-1] or bank_F.shape[0] != off[-1] \
            or bank_F.dim() != 2:
        raise ValueError('offset array does not match the bank arrays')
    prm = _register_params(voxel_size, clip_weight_thresh, inlier_feature_type, max_iter, max_break_count,
                           break_threshold_ratio, skip_refinement, safeguard, use_icp, ransac_hypotheses, ransac_seed)
    T, status, stats = _register_out(npairs)
    in_range = bool(((ids >= 0) & (ids < nfrag)).all())      # (out-of-range ids are the library's to report)
    n0 = int((off[ids[:, 0] + 1] - off[ids[:, 0]]).sum()) if in_range else None
    fl, ov = _register_hooks(forced_logit, override_idx1, n0, dev)
    check(lib.dgr_register_pairs(get_ctx(dev), inlier.handle, ptr(bank_coords), ptr(bank_xyz), ptr(bank_F),
                                 _np_ptr(off), nfrag, int(bank_F.shape[1]), _np_ptr(ids), npairs, C.byref(prm), ptr(ov),
                                 ptr(fl), _np_ptr(T), _np_ptr(status), _np_ptr(stats), stream_ptr(dev.index)))
    return _register_T64(lib, dev, npairs), status, stats


_BATCH_OUT = {'idx1': (0, torch.int64), 'logit': (1, torch.float32), 'weights': (2, torch.float32),
              'F0': (3, torch.float32), 'F1': (4, torch.float32)}


def batch_output(device, which):
    """Copy of a device-side intermediate of the last register_batch ('idx1', 'logit', 'weights',
    'F0', 'F1') as a flat torch tensor."""
    lib = _lib.load()
    dev = torch.device(device)
    wid, dtype = _BATCH_OUT[which]
    n = C.c_int64(0)
    check(lib.dgr_register_batch_output(get_ctx(dev), wid, None, 0, C.byref(n), stream_ptr(dev.index)))
    out = torch.empty(n.value, dtype=dtype, device=dev)
    check(lib.dgr_register_batch_output(get_ctx(dev), wid, ptr(out), out.numel() * out.element_size(),
                                        C.byref(n), stream_ptr(dev.index)))
    return out


def partition_stream(device, part, nparts):
    """A stream of the calling thread's context on share `part` of `nparts` (2 or 4) equal shares of the GPU's compute
    units (dgr_ctx_create_partition_stream, include/dgr_hip.h), as a torch stream: make it the current stream
    (`with torch.cuda.stream(s):`) for every call of this context.  `nparts = 1` drops the partition and returns None.
    Pays only when several contexts (one per host thread) keep the GPU busy at once; results do not depend on it."""
    device = torch.device(device)
    h = vp()
    check(_lib.load().dgr_ctx_create_partition_stream(get_ctx(device), int(part), int(nparts), C.byref(h)))
    return torch.cuda.ExternalStream(h.value, device) if h.value else None


def set_profiling(device, enable):
    check(_lib.load().dgr_ctx_set_profiling(get_ctx(device), int(bool(enable))))


def stage_times(device):
    t = (C.c_float * 16)()
    n = C.c_int(0)
    check(_lib.load().dgr_ctx_stage_times_v2(get_ctx(device), t, 16, C.byref(n)))
    names = ['fcgf', 'knn', 'inlier_inputs', 'inlier_net', 'registration', 'maps_3d', 'maps_6d', 'conv_kernels', 'o3d_steps']
    out = dict(zip(names, [float(v) for v in t[:n.value]]))
    out['conv_launches'] = int(_lib.load().dgr_ctx_conv_launches(get_ctx(device)))
    return out


def conv_launch_times(device):
    """Per-launch durations (ms) of the sparse-conv layers of the last profiled batch in launch order:
    (MFMA phase + reduce phase, MFMA phase alone)."""
    cap = 4096
    t, g = (C.c_float * cap)(), (C.c_float * cap)()
    n = C.c_int64(0)
    check(_lib.load().dgr_ctx_conv_launch_times(get_ctx(device), t, g, cap, C.byref(n)))
    return [float(t[i]) for i in range(n.value)], [float(g[i]) for i in range(n.value)]


def conv_launch_kernel_us(device):
    """Per launch of `conv_launch_times`: the kernel's own execution span in us (stamped by the kernel on the device wall
    clock: the duration rocprofv3 --kernel-trace reports, valid under concurrent streams); 0 = kernel not instrumented."""
    cap = 4096
    t = (C.c_float * cap)()
    n = C.c_int64(0)
    check(_lib.load().dgr_ctx_conv_launch_kernel_us(get_ctx(device), t, cap, C.byref(n)))
    return [float(t[i]) for i in range(n.value)]


def conv_launch_kinds(device):
    """Kernel variant (rocprof kernel name) of every launch reported by `conv_launch_times`."""
    cap = 1 << 16
    buf = C.create_string_buffer(cap)
    n = C.c_int64(0)
    check(_lib.load().dgr_ctx_conv_launch_kinds(get_ctx(device), buf, cap, C.byref(n)))
    names = buf.value.decode().split('\n')
    return names[:n.value]


def debug_ortho2rotation(p6, grad_R=None):
    """ortho2rotation forward (and backward for `grad_R` [n,3,3]) exactly as the registration kernel computes it."""
    dev = _dev(p6)
    p6 = _as(p6, torch.float32, dev).reshape(-1, 6)
    n = p6.shape[0]
    R = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    g = dp = None
    if grad_R is not None:
        g = _as(grad_R, torch.float32, dev).reshape(n, 9)
        dp = torch.empty((n, 6), dtype=torch.float32, device=dev)
    check(_lib.load().dgr_debug_ortho2rotation(get_ctx(dev), ptr(p6), n, ptr(g), ptr(R), ptr(dp), stream_ptr(dev.index)))
    return (R, dp) if grad_R is not None else R


def debug_smooth_l1(X, Y, quantization_size):
    """HighDimSmoothL1Loss per point, the device function of the registration kernel."""
    dev = _dev(X)
    X, Y = _as(X, torch.float32, dev), _as(Y, torch.float32, dev)
    out = torch.empty(X.shape[0], dtype=torch.float32, device=dev)
    check(_lib.load().dgr_debug_smooth_l1(get_ctx(dev), ptr(X), ptr(Y), X.shape[0], float(quantization_size), ptr(out),
                                          stream_ptr(dev.index)))
    return out
