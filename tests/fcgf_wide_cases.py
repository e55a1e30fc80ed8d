"""Inputs of tests/test_gpu_fcgf_wide.py: small 3-D clouds whose two coarse levels (tensor strides 4 and 8) put the
rule-major lists derived from the neighbour tables, and the tile walk of the wide conv kernel over them, at their edges.

The 128 / 256-channel layers of the FCGF net run on three maps: 'same' at ts 4, 'same' at ts 8 and 'down' at ts 4
(level 2 -> 3).  A tile is up to 64 pairs of ONE offset; a persistent workgroup walks an XCD-aware share of the tiles.
Every case states its edge as a precondition on the ORACLE's maps (`Case.pre`, asserted on the CPU by
tests/test_fcgf_wide_cases_cpu.py): a case that stops reaching its edge fails there, not silently on the GPU.

  a  two clouds of about 2 000 voxels: a level 3 of a few dozen rows, every offset of the two level-3 maps ('same' at
     ts 8, 'down' at ts 4) below 64 pairs -- every tile of theirs is partial;
  b1 a thin bar along x: the level-3 map has offsets with no pair at all (tile_ptr does not move over them);
  b2 one 8^3 cell: a single level-3 row, the centre offset only;
  c  one cloud of about 20 000 voxels: every level-2 offset holds several full tiles and a partial one, the offsets of
     the strided map lie on both sides of 128 pairs, and a workgroup of a 64-workgroup grid walks several tiles.

A batch whose last cloud is EMPTY at level 3 does not exist: a cloud is the set of rows with its batch index, every row
has a parent voxel at every stride, so a cloud with a row has a level-3 row, and a cloud without rows is not in the
input at all (the library takes coordinates, not per-cloud counts).  The nearest edge -- a cloud that is a single
level-3 row -- is the second cloud of case b2."""
import numpy as np

import maps_ref as ref
from helpers import random_cloud_coords

SEED = 23          # of the synthetic FCGF checkpoint the cases run through
CONV1_KS = 3
MAPS = (('same', 4), ('same', 8), ('down', 4))     # the lists a forward derives from its tables
# layers (forward order) that run on the wide kernel, with their map
WIDE_LAYERS = {7: ('same', 4), 8: ('same', 4), 9: ('down', 4), 10: ('same', 8), 11: ('same', 8), 13: ('same', 4), 14: ('same', 4)}


def share_walk(tiles):
    """tiles of the busiest workgroup of a 64-workgroup grid: an XCD gets ceil(T / 8) tiles, its eight workgroups deal them"""
    return -(-(-(-tiles // 8)) // 8)


def per_rule(o, kind, ts):
    return np.bincount(o.triplets(kind, ts)[0], minlength=27)


class Case:
    def __init__(self, name, make, pre):
        self.name, self.make, self._pre = name, make, pre
        self._coords = None

    @property
    def coords(self):
        if self._coords is None:
            c = np.ascontiguousarray(self.make(), np.int32)
            assert c.ndim == 2 and c.shape[1] == 4 and len(np.unique(c, axis=0)) == len(c)
            self._coords = c
        return self._coords

    def pre(self, oracle):
        self._pre(self, oracle)

    def __repr__(self):
        return self.name


_ORACLES = {}


def oracle_of(case):
    if case.name not in _ORACLES:
        _ORACLES[case.name] = ref.Oracle(case.coords, 3, CONV1_KS)
    return _ORACLES[case.name]


def _two_small():
    rng = np.random.default_rng(5)
    return np.concatenate([random_cloud_coords(rng, 9000, 8, 3, batch=0), random_cloud_coords(rng, 9000, 8, 3, batch=1)])


def _pre_two_small(case, o):
    c = case.coords
    assert sorted(set(c[:, 0].tolist())) == [0, 1] and 2500 <= len(c) <= 5000, len(c)
    assert 20 <= len(o.coords[8]) <= 200, len(o.coords[8])
    for kind, ts in (('same', 8), ('down', 4)):          # every tile of the level-3 maps is partial
        r = per_rule(o, kind, ts)
        assert 0 < r.max() < 64, (kind, ts, r)
    assert len(c) % 256 != 0 and len(o.coords[4]) % 64 != 0


def _bar():
    x = np.arange(-21, 44)
    g = np.stack(np.meshgrid(x, np.arange(2), np.arange(3), indexing='ij'), -1).reshape(-1, 3)
    return np.concatenate([np.zeros((len(g), 1), np.int64), g], axis=1)


def _pre_bar(case, o):
    r = per_rule(o, 'same', 8)
    n8 = len(o.coords[8])
    assert n8 >= 4 and sorted(np.nonzero(r)[0].tolist()) == [12, 13, 14] and r[13] == n8 and r[12] == r[14] == n8 - 1
    tile_ptr = np.concatenate([[0], np.cumsum(-(-r // 64))])
    assert (np.diff(tile_ptr) == 0).sum() == 24          # tile_ptr mostly flat
    assert (per_rule(o, 'down', 4) == 0).any()


def _one_cell():
    rng = np.random.default_rng(9)
    a = rng.permutation(512)[:150]
    cell = np.stack([a % 8, (a // 8) % 8, a // 64], axis=1)
    one = np.concatenate([np.zeros((len(cell), 1), np.int64), cell + np.array([-8, 16, -24])], axis=1)
    two = np.array([[1, 1, -5, 2], [1, 2, -5, 2]])       # a second cloud: two voxels, one row at every coarse level
    return np.concatenate([one, two])


def _pre_one_cell(case, o):
    c8 = o.coords[8]
    assert len(c8) == 2 and sorted(c8[:, 0].tolist()) == [0, 1]          # one level-3 row per cloud
    r = per_rule(o, 'same', 8)
    assert r[13] == 2 and r.sum() == 2                                   # the centre offset only
    assert (o.coords[8][-1, 0] == 1) and (o.coords[4][:, 0] == 1).sum() == 1


def _large():
    rng = np.random.default_rng(11)
    c = random_cloud_coords(rng, 36000, 52, 3)
    return c[:20011] if len(c) > 20011 else c


def _pre_large(case, o):
    assert 15000 <= len(case.coords) <= 20011 and len(case.coords) % 256 != 0, len(case.coords)
    r = per_rule(o, 'same', 4)
    assert (r > 128).all() and (r % 64 != 0).any(), r     # every level-2 offset: full tiles and a partial one
    d = per_rule(o, 'down', 4)
    assert ((d > 64) & (d < 128)).any() and (d > 128).any(), d          # the strided map crosses 64 and 128
    tiles = int((-(-r // 64)).sum())
    assert share_walk(tiles) >= 3, tiles                 # several tiles per workgroup of a 64-workgroup grid
    assert tiles > 256                                   # ... and more tiles than workgroups on the whole GPU
    r8 = per_rule(o, 'same', 8)
    assert (r8 > 64).any() and (r8 % 64 != 0).any()


CASES = [Case('a_two_small', _two_small, _pre_two_small), Case('b1_bar', _bar, _pre_bar),
         Case('b2_one_cell', _one_cell, _pre_one_cell), Case('c_large', _large, _pre_large)]
