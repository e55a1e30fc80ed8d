"""Plain numpy reference of ONE conv layer of ResUNetBN2C as the forward runs it, and of the pieces the layers hand to
each other (CPU only; used by tests/test_layer_trace_cpu.py and tests/test_gpu_layer_trace.py).

  * split2 / row_scale_of / row_amax_bits: csrc/split.h restated with np.float16 round-to-nearest;
  * encode / decode of the 6-D split rows (dgr_split_row_offset) and of the 3-D dense split rows (DESIGN.md section 3,
    conv_dense.hip), decoders returning (h + m) / scale in float64;
  * LAYERS: the 23 convs in forward order with their input, kernel map, residual and ReLU flags (the LAYERS table
    of net.hip);
  * unit_truth: float64 output of one layer and the per-element magnitude bound B = |shift| + sum |x||W| + |res|;
  * unit_norm: v / (|v| + 1e-8) with B propagated to first order;
  * unit_f32: the same layer in the reference's own float32 arithmetic (oracle.resunet.sparse_conv + batch_norm), the
    yardstick the device error is measured against.
"""
import numpy as np
import torch

from oracle import resunet as oresunet

BN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# split.h
# ---------------------------------------------------------------------------------------------------------------------
def row_scale_of(max_abs_bits):
    """dgr_row_scale_of: the power of two that moves a row's largest |x| (given as bits) into [2^14, 2^15); biased
    exponent clamped to [20, 240]; a zero row gets 1."""
    b = np.asarray(max_abs_bits, np.uint32)
    e = np.clip(b >> np.uint32(23), 20, 240).astype(np.uint32)
    s = ((np.uint32(268) - e) << np.uint32(23)).astype(np.uint32).view(np.float32)
    return np.where(b == 0, np.float32(1), s).astype(np.float32)


def row_amax_bits(x, relu):
    """Integer maximum over each row of the bit patterns of max(x, 0) (pending ReLU) or |x|: what a producer's epilogue
    leaves in amax[row]."""
    x = np.ascontiguousarray(x, np.float32)
    if relu:
        x = np.maximum(x, np.float32(0))
    bits = x.view(np.uint32) & np.uint32(0x7fffffff)
    return bits.max(axis=1).astype(np.uint32)


def split2(x, sx):
    """dgr_split2: s x = h + m, two f16 pieces by round-to-nearest (sx a power of two, broadcast over x)."""
    with np.errstate(over='ignore', invalid='ignore'):
        xs = (np.asarray(x, np.float32) * np.asarray(sx, np.float32)).astype(np.float32)
        h = xs.astype(np.float16)
        m = (xs - h.astype(np.float32)).astype(np.float16)
    return h, m


def _relu32(x, relu):
    x = np.ascontiguousarray(x, np.float32)
    # the device applies a pending ReLU as an integer max of the bit pattern with 0: -0.0 becomes +0.0
    return np.where(x > 0, x, np.float32(0)).astype(np.float32) if relu else x


# ---- 6-D split rows: per 64-channel block 128 bytes of h, then 128 bytes of m (dgr_split_row_offset)
def encode_split6(x, relu):
    """-> (planes uint8 [n, 4 C], scale f32 [n]) as reduce_rows_kernel<., true> writes them."""
    x = _relu32(x, relu)
    n, c = x.shape
    assert c % 64 == 0
    scale = row_scale_of(row_amax_bits(x, False))
    h, m = split2(x, scale[:, None])
    planes = np.stack([h.reshape(n, c // 64, 64), m.reshape(n, c // 64, 64)], axis=2)   # [n, blocks, piece, 64]
    return np.ascontiguousarray(planes).view(np.uint8).reshape(n, 4 * c), scale


def decode_split6(planes, scale):
    """-> float64 [n, C]: (h + m) / scale."""
    n = planes.shape[0]
    c = planes.shape[1] // 4
    p = np.ascontiguousarray(planes).view(np.float16).reshape(n, c // 64, 2, 64).astype(np.float64)
    return (p[:, :, 0, :] + p[:, :, 1, :]).reshape(n, c) / np.asarray(scale, np.float64)[:, None]


# ---- 3-D dense split rows: [h plane: C halves][m plane: C halves]; inside a plane every 32-channel group s in the
# dense-tile kernel's gather order: 16-byte chunk c (0..3) = channels 32 s + 4 c .. + 3, then 32 s + 16 + 4 c .. + 3
def dense_channel_order(c):
    j = np.arange(c)
    s, r = j // 32, j % 32
    chunk, e = r // 8, r % 8
    return 32 * s + 16 * (e // 4) + 4 * chunk + (e % 4)   # stored position j holds this channel


def encode_dense(x, relu):
    """-> (bytes uint8 [n, 4 C], amax uint32 [n]); the scale is dgr_row_scale_of(amax), not stored."""
    x = _relu32(x, relu)
    amax = row_amax_bits(x, False)
    h, m = split2(x, row_scale_of(amax)[:, None])
    order = dense_channel_order(x.shape[1])
    return np.ascontiguousarray(np.concatenate([h[:, order], m[:, order]], axis=1)).view(np.uint8), amax


def decode_dense(raw, amax):
    """-> float64 [n, C]: (h + m) / row_scale_of(amax)."""
    n = raw.shape[0]
    c = raw.shape[1] // 4
    p = np.ascontiguousarray(raw).view(np.float16).reshape(n, 2, c).astype(np.float64)
    out = np.empty((n, c), np.float64)
    out[:, dense_channel_order(c)] = p[:, 0, :] + p[:, 1, :]
    return out / row_scale_of(amax).astype(np.float64)[:, None]


def dense_planes(raw):
    """(h, m) f16 [n, C] of dense split rows, channels in natural order."""
    n = raw.shape[0]
    c = raw.shape[1] // 4
    p = np.ascontiguousarray(raw).view(np.float16).reshape(n, 2, c)
    inv = np.empty(c, np.int64)
    inv[dense_channel_order(c)] = np.arange(c)
    return p[:, 0, inv], p[:, 1, inv]


def resplit_mismatches(h, m):
    """Elements whose pieces are NOT what dgr_split2 makes of their own value v = h + m (exact in f32): the number of
    elements where split2(v) differs from (h, m).  Two cases are the same split and do not count: a residual that
    underflowed to a zero of either sign, and an exact tie |v - h| = half a step of h, which round-to-nearest-even
    may resolve to the other neighbour when it sees v instead of the original product (then m must still be v - h)."""
    v = h.astype(np.float32) + m.astype(np.float32)
    assert (v.astype(np.float64) == h.astype(np.float64) + m.astype(np.float64)).all()
    h2, m2 = split2(v, np.float32(1))
    same = (h2 == h) & (m2 == m)   # by value: -0 == +0
    tie = (h2 != h) & (np.abs(v - h.astype(np.float32)) == np.abs(v - h2.astype(np.float32))) & \
        ((v - h.astype(np.float32)).astype(np.float16) == m)
    return int((~(same | tie)).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the 23 layers as the forward runs them (net.hip, the LAYERS and TENSORS tables)
# ---------------------------------------------------------------------------------------------------------------------
# pending ReLU of every tensor (consumers apply max(x, 0) when reading)
RELU = {'X': 0, 'H': 1, 'OUT': 0, 'CAT4': 1, 'CAT2': 1, 'CAT1': 1}
for _l in ('1', '2', '4', '8'):
    RELU.update({'T' + _l: 0, 'Y' + _l: 1, 'S' + _l: 1, 'U' + _l: 0, 'V' + _l: 1, 'S' + _l + 'T': 1})
# tensor stride of every tensor's coordinate map
STRIDE = {n: int(n[1]) for n in RELU if n[0] in 'TYSUV'}
STRIDE.update({'X': 1, 'H': 1, 'OUT': 1, 'CAT4': 4, 'CAT2': 2, 'CAT1': 1})
# the concatenation buffers: decoder half first (ME.cat((out_s*_tr, out_s*)))
CAT = {'CAT4': ('S4T', 'S4'), 'CAT2': ('S2T', 'S2'), 'CAT1': ('S1T', 'S1')}


def _block(name, a, y, s, ts):
    return [dict(name=name + '.conv1', norm=name + '.norm1', inp=a, map=('same', ts), out=y, res=None),
            dict(name=name + '.conv2', norm=name + '.norm2', inp=y, map=('same', ts), out=s, res=a)]


LAYERS = ([dict(name='conv1', norm='norm1', inp='X', map=('conv1', 1), out='T1', res=None)] + _block('block1', 'T1', 'Y1', 'S1', 1) +
          [dict(name='conv2', norm='norm2', inp='S1', map=('down', 1), out='T2', res=None)] + _block('block2', 'T2', 'Y2', 'S2', 2) +
          [dict(name='conv3', norm='norm3', inp='S2', map=('down', 2), out='T4', res=None)] + _block('block3', 'T4', 'Y4', 'S4', 4) +
          [dict(name='conv4', norm='norm4', inp='S4', map=('down', 4), out='T8', res=None)] + _block('block4', 'T8', 'Y8', 'S8', 8) +
          [dict(name='conv4_tr', norm='norm4_tr', inp='S8', map=('up', 8), out='U4', res=None)] + _block('block4_tr', 'U4', 'V4', 'S4T', 4) +
          [dict(name='conv3_tr', norm='norm3_tr', inp='CAT4', map=('up', 4), out='U2', res=None)] + _block('block3_tr', 'U2', 'V2', 'S2T', 2) +
          [dict(name='conv2_tr', norm='norm2_tr', inp='CAT2', map=('up', 2), out='U1', res=None)] + _block('block2_tr', 'U1', 'V1', 'S1T', 1) +
          [dict(name='conv1_tr', norm=None, inp='CAT1', map=None, out='H', res=None),
           dict(name='final', norm=None, inp='H', map=None, out='OUT', res=None)])
assert len(LAYERS) == 23


def layer_map(maps, L):
    """(kernel map (k, in, out) | None for the identity map, number of output rows) from oracle.resunet.SparseMaps."""
    n_out = len(maps.coords[STRIDE[L['out']]])
    if L['map'] is None:
        return None, n_out
    kind, ts = L['map']
    km = maps.same(1, maps.conv1_ks) if kind == 'conv1' else maps.same(ts) if kind == 'same' else \
        maps.down(ts) if kind == 'down' else maps.up(ts)
    return km, n_out


def folded(sd, L, dtype=np.float64):
    """The layer's folded weights W gamma / sqrt(sigma^2 + 1e-5) [K, Cin, Cout] and its shift [Cout]."""
    W = np.asarray(sd[L['name'] + '.kernel'], dtype)
    if W.ndim == 2:
        W = W[None]
    cout = W.shape[2]
    shift = np.zeros(cout, dtype)
    if L['norm']:
        p = L['norm'] + '.bn.'
        g, b = np.asarray(sd[p + 'weight'], dtype), np.asarray(sd[p + 'bias'], dtype)
        m, v = np.asarray(sd[p + 'running_mean'], dtype), np.asarray(sd[p + 'running_var'], dtype)
        s = g / np.sqrt(v + dtype(BN_EPS))
        W = W * s[None, None, :]
        shift = b - m * s
    if L['name'] + '.bias' in sd:
        shift = shift + np.asarray(sd[L['name'] + '.bias'], dtype).reshape(-1)
    return W, shift


def unit_truth(x, kmap, n_out, Wf, shift, in_relu, res=None, res_relu=False):
    """One layer in float64: y[o] = shift + sum over the map's pairs (k, i, o) of max(x[i], 0)? @ Wf[k] (+ max(res, 0)?),
    the identity map when kmap is None.  Returns (y, B), B = |shift| + sum |x| @ |Wf| + |res| per element: the
    magnitude an evaluation's rounding error is relative to."""
    x = np.asarray(x, np.float64)
    if in_relu:
        x = np.maximum(x, 0)
    y = np.tile(np.asarray(shift, np.float64), (n_out, 1))
    B = np.abs(y)
    if kmap is None:
        y += x @ Wf[0]
        B += np.abs(x) @ np.abs(Wf[0])
    else:
        k, i, o = kmap
        for kk in np.unique(k):
            sel = k == kk
            np.add.at(y, o[sel], x[i[sel]] @ Wf[kk])
            np.add.at(B, o[sel], np.abs(x[i[sel]]) @ np.abs(Wf[kk]))
    if res is not None:
        r = np.asarray(res, np.float64)
        if res_relu:
            r = np.maximum(r, 0)
        y += r
        B += np.abs(r)
    return y, B


def unit_norm(v, B):
    """n = v / (|v|_2 + 1e-8) per row, and the bound of n to first order in a perturbation dv with |dv_j| <= B_j:
        dn_j = dv_j / s - v_j (v . dv) / (|v| s^2),  s = |v| + 1e-8
        =>  |dn_j| <= B_j / s + |v_j| (sum_i |v_i| B_i) / (|v| s^2)."""
    v = np.asarray(v, np.float64)
    nv = np.sqrt((v * v).sum(axis=1, keepdims=True))
    s = nv + 1e-8
    Bn = B / s + np.abs(v) * (np.abs(v) * B).sum(axis=1, keepdims=True) / (np.maximum(nv, 1e-300) * s * s)
    return v / s, Bn


def unit_f32(x, kmap, n_out, sd, L, in_relu, res=None, res_relu=False, normalize=False):
    """The same layer in the reference's float32 arithmetic: oracle.resunet.sparse_conv, then batch_norm, then the
    residual (model/residual_block.py:118-134); the k = 1 layers as a matrix product (+ bias, + unit norm)."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if in_relu:
        t = torch.relu(t)
    sd32 = {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in sd.items()
            if k.startswith(L['name'] + '.') or (L['norm'] and k.startswith(L['norm'] + '.'))}
    w = sd32[L['name'] + '.kernel']
    if kmap is None:
        y = t @ (w if w.dim() == 2 else w[0])
        if L['name'] + '.bias' in sd32:
            y = y + sd32[L['name'] + '.bias'].reshape(1, -1)
    else:
        y = oresunet.sparse_conv(t, kmap, w, n_out)
    if L['norm']:
        y = oresunet.batch_norm(y, sd32, L['norm'])
    if res is not None:
        r = torch.from_numpy(np.ascontiguousarray(res, np.float32))
        y = y + (torch.relu(r) if res_relu else r)
    if normalize:
        y = y / (torch.norm(y, p=2, dim=1, keepdim=True) + 1e-8)
    return y.numpy()


def run_unit(maps, sd, L, x, res=None, normalize=False, with_f32=True):
    """(y64, B, e32) of layer L on input x (and residual res): the float64 truth, its bound and the float32
    reference's own largest |y32 - y64| / B on this very unit and input."""
    km, n_out = layer_map(maps, L)
    Wf, shift = folded(sd, L)
    in_relu, res_relu = RELU[L['inp']], (RELU[L['res']] if L['res'] else 0)
    y, B = unit_truth(x, km, n_out, Wf, shift, in_relu, res, res_relu)
    if normalize:
        y, B = unit_norm(y, B)
    e32 = None
    if with_f32:
        y32 = unit_f32(x, km, n_out, sd, L, in_relu, res, res_relu, normalize)
        e32 = float((np.abs(y32.astype(np.float64) - y) / np.maximum(B, 1e-300)).max())
    return y, B, e32
