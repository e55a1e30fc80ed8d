"""CPU tests of tests/layer_trace_ref.py, the numpy reference the per-layer GPU parity test
(tests/test_gpu_layer_trace.py) compares the device with: the f16-piece split and its two row layouts, one layer in
float64 with its magnitude bound, and the 23 layers chained against the oracle's float64 forward."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import layer_trace_inputs as inp   # noqa: E402
import layer_trace_ref as ref   # noqa: E402
from oracle import resunet as oresunet   # noqa: E402


def _rows(rng, n, c):
    x = rng.uniform(-2, 2, (n, c)).astype(np.float32)
    x *= (10.0 ** ((np.arange(n) % 13) - 6.0))[:, None].astype(np.float32)   # row magnitudes 1e-6 .. 1e6
    x[:, 3::7] *= np.float32(1e-5)                                            # small channels inside every row
    x[2] = 0
    x[3] = -np.abs(x[3])                                                      # all negative: zero under ReLU
    return x


def test_row_scale_of_exponent_clamps():
    f = lambda v: np.array([v], np.float32).view(np.uint32)   # noqa: E731
    assert ref.row_scale_of(np.uint32(0)) == 1.0
    for v in (3.0, 1.0, 1e-3, 7e5, 1.9999999):
        s = float(ref.row_scale_of(f(v))[0])
        assert 2.0 ** 14 <= v * s < 2.0 ** 15 and np.log2(s) == np.round(np.log2(s))
    # biased exponent clamped to [20, 240]: denormal / tiny rows and rows near the f32 limit get a finite scale
    assert ref.row_scale_of(f(1e-41))[0] == np.float32(2.0 ** (141 - 20))
    assert ref.row_scale_of(f(2.0 ** -120))[0] == np.float32(2.0 ** (141 - 20))
    assert ref.row_scale_of(f(2.0 ** (20 - 127)))[0] == np.float32(2.0 ** (141 - 20))
    assert ref.row_scale_of(f(2.0 ** (21 - 127)))[0] == np.float32(2.0 ** (141 - 21))
    assert ref.row_scale_of(f(3e38))[0] == np.float32(2.0 ** (141 - 240))
    assert ref.row_scale_of(f(2.0 ** (240 - 127)))[0] == np.float32(2.0 ** (141 - 240))
    assert ref.row_scale_of(f(2.0 ** (239 - 127)))[0] == np.float32(2.0 ** (141 - 239))


def test_row_amax_bits():
    x = np.array([[1.0, -4.0, 2.0, -0.0], [-1.0, -2.0, -3.0, -0.5]], np.float32)
    assert ref.row_amax_bits(x, False).tolist() == np.array([4.0, 3.0], np.float32).view(np.uint32).tolist()
    assert ref.row_amax_bits(x, True).tolist() == np.array([2.0, 0.0], np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('c', [64, 128, 256])
def test_split6_roundtrip_and_layout(c, relu):
    x = _rows(np.random.default_rng(c + relu), 40, c)
    planes, scale = ref.encode_split6(x, relu)
    assert planes.shape == (40, 4 * c) and planes.dtype == np.uint8
    xr = np.maximum(x, 0) if relu else x
    rowmax = np.abs(xr).max(axis=1, keepdims=True).astype(np.float64)
    dec = ref.decode_split6(planes, scale)
    assert (np.abs(dec - xr) <= 2.0 ** -22 * rowmax).all()
    assert (dec[2] == 0).all() and scale[2] == 1.0
    if relu:
        assert (dec[3] == 0).all() and scale[3] == 1.0 and not planes[3].any()
    # the layout, stated independently: byte offset of channel ch of piece p (dgr_split_row_offset)
    h, m = ref.split2(xr, scale[:, None])
    for ch in (0, 1, 63, c - 64, c - 1):
        for p, piece in ((0, h), (1, m)):
            off = (ch >> 6) * 256 + p * 128 + (ch & 63) * 2
            assert (planes[:, off:off + 2].copy().view(np.float16)[:, 0].view(np.uint16) == piece[:, ch].view(np.uint16)).all()


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('c', [32, 64])
def test_dense_split_roundtrip_and_layout(c, relu):
    x = _rows(np.random.default_rng(10 * c + relu), 40, c)
    raw, amax = ref.encode_dense(x, relu)
    assert raw.shape == (40, 4 * c) and raw.dtype == np.uint8
    xr = np.maximum(x, 0) if relu else x
    assert (amax == ref.row_amax_bits(x, relu)).all()
    rowmax = np.abs(xr).max(axis=1, keepdims=True).astype(np.float64)
    dec = ref.decode_dense(raw, amax)
    assert (np.abs(dec - xr) <= 2.0 ** -22 * rowmax).all()
    assert (dec[2] == 0).all() and amax[2] == 0
    if relu:
        assert (dec[3] == 0).all() and amax[3] == 0 and not raw[3].any()
    # the pieces are the split of their own value (h + m is exact in f32), and a wrong piece is seen
    hh, mm = ref.dense_planes(raw)
    assert (dec.astype(np.float32) == dec).all() and ref.resplit_mismatches(hh, mm) == 0
    bad = mm.copy()
    j = int(np.argmax(np.abs(hh[5])))
    bad[5, j] = np.float16(float(bad[5, j]) + float(abs(hh[5, j])) * 2.0 ** -9)
    assert ref.resplit_mismatches(hh, bad) == 1
    # the layout, stated independently (conv_dense.hip): plane p at byte 2 C p; 32-channel group s at + 64 s; 16-byte
    # chunk q holds channels 32 s + 4 q .. + 3 and 32 s + 16 + 4 q .. + 3
    h, m = ref.split2(xr, ref.row_scale_of(amax)[:, None])
    halves = raw.view(np.uint16)
    for p, piece in ((0, h), (1, m)):
        for s in range(c // 32):
            for q in range(4):
                for e in range(8):
                    ch = 32 * s + 4 * q + (e & 3) + (16 if e >= 4 else 0)
                    assert (halves[:, p * c + 32 * s + 8 * q + e] == piece[:, ch].view(np.uint16)).all()


def test_up_two_voxels_by_hand():
    """Two fine voxels under one coarse voxel: the transposed conv sends the coarse row through the centre offset
    (k = 13) to the fine voxel at the coarse corner and through offset (+1, 0, 0) (k = 14) to its neighbour."""
    fine = np.array([[0, -2, 0, 4], [0, -1, 0, 4]], np.int32)
    maps = oresunet.SparseMaps(fine, 3, 3)
    assert maps.coords[2].tolist() == [[0, -2, 0, 4]]
    k, i, o = maps.up(2)
    assert sorted(zip(k.tolist(), i.tolist(), o.tolist())) == [(13, 0, 0), (14, 0, 1)]
    W = np.zeros((27, 2, 2))
    W[13] = [[1, 2], [3, 4]]
    W[14] = [[-1, 0.5], [2, -8]]
    W[12] = 99.0   # an offset that has no pair here
    shift = np.array([0.25, -1.0])
    x = np.array([[2.0, -3.0]])
    y, B = ref.unit_truth(x, (k, i, o), 2, W, shift, False)
    assert y.tolist() == [[0.25 + 2 - 9, -1 + 4 - 12], [0.25 - 2 - 6, -1 + 1 + 24]]
    assert B.tolist() == [[0.25 + 2 + 9, 1 + 4 + 12], [0.25 + 2 + 6, 1 + 1 + 24]]
    y, B = ref.unit_truth(x, (k, i, o), 2, W, shift, True, res=np.array([[-1.0, 1.0], [5.0, -5.0]]), res_relu=True)
    assert y.tolist() == [[0.25 + 2, -1 + 4 + 1], [0.25 - 2 + 5, -1 + 1]]
    assert B.tolist() == [[0.25 + 2, 1 + 4 + 1], [0.25 + 2 + 5, 1 + 1]]


def test_unit_norm_bound_is_first_order():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(50, 16))
    B = np.abs(v) + rng.uniform(0, 1, v.shape)
    n, Bn = ref.unit_norm(v, B)
    np.testing.assert_allclose(n, v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-8), rtol=1e-15)
    for _ in range(20):   # any perturbation inside the box moves n by at most eps * Bn (+ second order)
        eps = 1e-7
        dv = eps * B * rng.choice([-1.0, 1.0], v.shape)
        n2 = (v + dv) / (np.linalg.norm(v + dv, axis=1, keepdims=True) + 1e-8)
        assert (np.abs(n2 - n) <= eps * Bn * (1 + 1e-4)).all()


def chain(maps, sd, x, normalize):
    """All 23 layers through unit_truth, each fed the previous ones' signed outputs."""
    t = {'X': np.asarray(x, np.float64)}
    for L in ref.LAYERS:
        for cat, halves in ref.CAT.items():
            if L['inp'] == cat:
                t[cat] = np.concatenate([t[halves[0]], t[halves[1]]], axis=1)
        y, B, _ = ref.run_unit(maps, sd, L, t[L['inp']], t[L['res']] if L['res'] else None,
                               normalize and L['name'] == 'final', with_f32=False)
        assert y.shape == B.shape and (B >= np.abs(y) * (1 - 1e-12)).all()
        t[L['out']] = y
    return t


@pytest.mark.parametrize('net,cloud', [('fcgf32', 'D'), ('rule12', 'C'), ('inl6', 'C6')])
def test_chained_units_reproduce_the_f64_forward(net, cloud):
    D, cin, cout, ks, norm, _, _ = inp.NETS[net]
    sd = inp.state_dict(net)
    coords = inp.clouds()[cloud]
    x = inp.feats(net, cloud, len(coords))
    out, inter = oresunet.resunet_forward(sd, coords, x, D, ks, norm, return_intermediates=True, dtype=torch.float64)
    t = chain(oresunet.SparseMaps(coords, D, ks), sd, x, norm)
    got = {'s1': t['S1'], 's2': t['S2'], 's4': t['S4'], 's8': t['S8'], 's4_tr': t['S4T'], 's2_tr': t['S2T'],
           's1_tr': t['S1T']}
    for name, v in got.items():   # the oracle's saved activations are post-ReLU
        r = np.asarray(inter[name], np.float64)
        assert np.abs(np.maximum(v, 0) - r).max() <= 1e-12 * max(np.abs(r).max(), 1e-300), name
    assert np.abs(t['OUT'] - out).max() <= 1e-12 * np.abs(out).max()
