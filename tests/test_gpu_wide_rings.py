"""The rings of the wide 6-D conv kernel (conv_wide.hip) at their edges: the compute waves' weight ring, the requesters'
gather sets, their index / scale registers and the index / scale rings in LDS all turn with the tiles a workgroup walks,
and their prologues and drains are exact only if a workgroup with 1, 2, 3 or D - 1, D, D + 1 tiles (D = a ring's depth in
tiles) still requests, publishes and lands every row in time.

Every case of tests/wide_rings_cases.py goes through all six (C_in, C_out) shapes of `dgr_conv_wide_supported`, one layer
at a time (`dgr_debug_conv_layer`, as tests/aux/split_f64_dump.py does for its `c6_*` tensors), and

  * states its edge and reaches it: asserted here from the library's own `tile_ptr` / `rule_ptr` (`ops.Maps.raw`);
  * agrees with the float64 statement of the layer (`layer_truth`, copied from tests/test_gpu_split_f64.py) under that
    test's bound: error <= max(1.5 x the exact-f32 kernel's error on the same input (DGR_EXACT_F32=1), 2e-7) of
    sum |x| |w|, per output row;
  * returns the same bytes twice on the plain stream, and on a CU-masked stream of 64 compute units (where the grid is
    64 workgroups and the case's busiest workgroup walks exactly the stated number of tiles).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import wide_rings_cases as wc   # noqa: E402
from oracle import me_semantics as me   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp('wide_rings')
    out = {}
    for name, env, args in (('split', {}, ['repro']), ('f32', {'DGR_EXACT_F32': '1'}, [])):
        e = {k: v for k, v in os.environ.items() if k != 'DGR_EXACT_F32'}
        e.update(env)
        path = str(d / f'{name}.npz')
        subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'aux', 'wide_rings_dump.py'), path] + args, env=e,
                       check=True, timeout=600)
        out[name] = np.load(path)
    return out


@pytest.fixture(scope='module')
def sd():
    from deepglobalregistration_amd import synth
    return synth.synth_state_dict(6, 6, 1, 3, wc.SEED)


_MAPS = {}


def kernel_map_of(case):
    if case.name not in _MAPS:
        _MAPS[case.name] = me.kernel_map(case.coords, case.coords, 6, 3, 1)
    return _MAPS[case.name]


def layer_truth(sd, name, norm, case, x):
    """f64: out[o] = shift + sum over the 3^D map of x[i] @ (W[k] * scale), and the magnitude bound
    sum |x| @ |W * scale| per output element (the scale an f32 evaluation's rounding error is relative to)."""
    W = np.asarray(sd[name + '.kernel'], np.float64)
    g, b = np.asarray(sd[norm + '.bn.weight'], np.float64), np.asarray(sd[norm + '.bn.bias'], np.float64)
    m, v = np.asarray(sd[norm + '.bn.running_mean'], np.float64), np.asarray(sd[norm + '.bn.running_var'], np.float64)
    s = g / np.sqrt(v + 1e-5)
    Wf = W * s[None, None, :]
    shift = b - m * s
    xx = np.asarray(x, np.float64)
    k, i, o = kernel_map_of(case)
    n = len(case.coords)
    out = np.tile(shift, (n, 1))
    bound = np.tile(np.abs(shift), (n, 1))
    for kk in np.unique(k):
        sel = k == kk
        np.add.at(out, o[sel], xx[i[sel]] @ Wf[kk])
        np.add.at(bound, o[sel], np.abs(xx[i[sel]]) @ np.abs(Wf[kk]))
    return out, bound


@pytest.mark.parametrize('case', wc.CASES, ids=repr)
def test_case_reaches_its_edge(case):
    from deepglobalregistration_amd import ops
    m = ops.Maps(case.coords, 6, lean=True)
    tile_ptr, rule_ptr = m.raw('same', 1, 'tile_ptr'), m.raw('same', 1, 'rule_ptr')
    rules = np.diff(rule_ptr[:wc.K + 1])
    tiles = int(tile_ptr[wc.K])
    assert (np.diff(tile_ptr[:wc.K + 1]) == (rules + 63) // 64).all()   # a tile = up to 64 pairs of one rule
    assert int(rule_ptr[wc.K]) == len(kernel_map_of(case)[0])
    if case.tiles is not None:
        assert tiles == case.tiles
    # 64 workgroups, eight per XCD: XCD x owns tiles [x per, (x + 1) per), its workgroup j walks those with index = j mod 8
    per = -(-tiles // 8)
    walks = [len(range(x * per + j, min(tiles, (x + 1) * per), 8)) for x in range(8) for j in range(8)]
    assert max(walks) == case.walk == wc.share_walk(tiles)
    if case.name == 'tiles5':
        assert tiles < 8 and sum(1 for x in range(8) if x * per >= tiles) == 3      # three XCD ranges are empty
    if case.name == 'tiles9':
        assert tiles == 9 and [min(tiles, (x + 1) * per) - min(tiles, x * per) for x in range(8)] == [2, 2, 2, 2, 1, 0, 0, 0]
    assert set(case.rule_sizes) <= set(rules.tolist())
    if case.walk >= 31:
        assert rules.max() > 64 * 8                                          # rules of many full tiles


@pytest.mark.parametrize('shape', wc.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('case', wc.CASES, ids=repr)
def test_against_f64_and_reproducible(dumps, sd, case, shape):
    cin, cout, _, name, norm = shape
    key = f'{case.name}/{cin}x{cout}'
    truth, bound = layer_truth(sd, name, norm, case, case.features(cin))
    rb = bound.max(axis=1)
    res = {}
    for mode in ('split', 'f32'):
        y = np.asarray(dumps[mode][key], np.float64)
        assert y.shape == truth.shape and np.isfinite(y).all(), mode
        res[mode] = float((np.abs(y - truth).max(axis=1) / rb).max())
    print(f'{key:28s} max over rows of max|y - f64| / max sum|x||w|:  split {res["split"]:.2e}   exact-f32 {res["f32"]:.2e}')
    assert res['split'] <= max(1.5 * res['f32'], 2e-7), (key, res)
    assert int(dumps['split'][key + '/again']) == 1, 'two runs on the plain stream differ'
    assert int(dumps['split'][key + '/share']) == 1, 'the run on a 64-CU share differs from the whole GPU'
