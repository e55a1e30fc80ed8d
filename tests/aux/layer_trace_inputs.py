"""Seeded nets and clouds shared by tests/test_gpu_layer_trace.py (float64 side) and tests/aux/layer_trace_dump.py
(device side): the smallest clouds that still reach every row-block edge of the conv kernels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import random_cloud_coords   # noqa: E402
from deepglobalregistration_amd import synth   # noqa: E402

# name -> (D, cin, cout, conv1 kernel size, normalize, seed, clouds)
NETS = {
    'fcgf32': (3, 1, 32, 7, True, 41, ('A', 'B', 'C', 'D')),
    'fcgf16': (3, 1, 16, 5, False, 42, ('A', 'B', 'C', 'D')),
    'rule12': (3, 12, 16, 3, False, 43, ('D',)),                 # rule-major 3-D path (more than 8 input channels)
    'inl6': (6, 6, 1, 3, False, 44, ('A6', 'C6', 'D6')),
    'inl1': (6, 1, 1, 3, False, 45, ('A6', 'C6', 'D6')),
}


def state_dict(net):
    D, cin, cout, ks, _, seed, _ = NETS[net]
    return synth.synth_state_dict(D, cin, cout, ks, seed)


def _pairs6(c0, rng, spread):
    c1 = c0[:, 1:] + rng.integers(-spread, spread + 1, (len(c0), 3)).astype(np.int32)
    return np.concatenate([c0, c1], axis=1).astype(np.int32)


def clouds():
    rng = np.random.default_rng(77)
    out = {}
    # A: one voxel at negative coordinates
    out['A'] = np.array([[0, -3, -5, -2]], np.int32)
    # B: the full 8 x 8 x 8 cube at a negative origin: 512 / 64 / 8 / 1 rows per level, interior rows own all 27
    # offsets, all eight parity classes equally full
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing='ij'), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))] + np.array([-8, -16, -8])
    out['B'] = np.concatenate([np.zeros((512, 1), np.int64), g], axis=1).astype(np.int32)
    # C: the first 129 rows of a random two-batch cloud: one 128-row workgroup plus one row, ragged parity classes
    c = np.concatenate([random_cloud_coords(rng, 90, 5, 3, batch=0), random_cloud_coords(rng, 120, 5, 3, batch=1)])
    assert len(c) >= 129 and c[128, 0] == 1
    out['C'] = np.ascontiguousarray(c[:129])
    # D: a two-batch surface cloud, N no multiple of 64
    d = np.concatenate([random_cloud_coords(rng, 420, 9, 3, batch=0), random_cloud_coords(rng, 420, 9, 3, batch=1)])
    if len(d) % 64 == 0:
        d = d[:-1]
    assert 600 <= len(d) <= 800 and len(d) % 64 != 0, len(d)
    out['D'] = np.ascontiguousarray(d)
    # A6: one row
    out['A6'] = np.array([[0, -1, 2, -3, 0, 3, -2]], np.int32)
    # C6: 65 pipeline-shaped rows (a unique 3-D voxel + a second 3-D voxel): the centre rule gets a 64-pair tile plus a
    # 1-pair tile
    c0 = random_cloud_coords(rng, 120, 4, 3)
    assert len(c0) >= 65
    out['C6'] = _pairs6(c0[:65], rng, 1)
    # D6: about 300 rows, small extent: the stride-8 level is dense
    c0 = random_cloud_coords(rng, 400, 5, 3)
    assert 200 <= len(c0) <= 400, len(c0)
    out['D6'] = _pairs6(c0, rng, 2)
    return out


def feats(net, cloud, n):
    """Input features [n, cin]: finite, both signs, seeded per (net, cloud)."""
    cin = NETS[net][1]
    rng = np.random.default_rng([NETS[net][5], sum(map(ord, cloud))])
    return np.cos(rng.uniform(-3, 3, (n, cin))).astype(np.float32)
