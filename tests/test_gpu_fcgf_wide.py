"""The 128 / 256-channel K = 27 layers of the 3-D FCGF net on the wide rule-major kernel (conv_wide.hip + reduce_rows)
over lists derived from the neighbour tables (kmap.hip, nbr_list_count / nbr_list_fill) -- the per-net option
`dgr_net_set_wide_coarse` (ops.NetHandle(..., wide_coarse=True)) that the product's model wrapper sets --, at the edges:
the cases of tests/fcgf_wide_cases.py, each pinned to its edge on the CPU (tests/test_fcgf_wide_cases_cpu.py).

  1. map contract: the lists read back raw equal tests/maps_ref.py from the oracle's triplets (integer equality), what a
     lean list map does not keep is refused, and two builds are bitwise equal;
  2. forward: every layer, per element, against the float64 unit reference of tests/layer_trace_ref.py on the input the
     device itself fed it, under the bound of tests/test_gpu_layer_trace.py for the split modes
     (|y - y64| <= (1.5 e32 + 2^-21) B; taken from there: `ADD`);
  3. kernel against kernel: every tensor against a child process with DGR_NO_WIDE3=1 (the output-stationary kernel),
     within the bound of tests/test_gpu_dense_conv.py (4e-6 of the tensor's largest value);
  4. two forwards, and one on a quarter share of the compute units, return the same bytes in every tensor;
  5. `conv_launch_kinds` names the wide kernel for exactly the seven layers, and for none with the switch set.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import fcgf_wide_cases as fc   # noqa: E402
import layer_trace_ref as ref   # noqa: E402
import maps_ref   # noqa: E402
from test_gpu_layer_trace import ADD, Forward   # noqa: E402  (the bound and the reader of a dumped forward)
from oracle import resunet as oresunet   # noqa: E402

pytestmark = pytest.mark.gpu
KERNEL_VS_KERNEL = 4e-6        # tests/test_gpu_dense_conv.py
SWITCHES = ('DGR_NO_WIDE3', 'DGR_OS_LISTS', 'DGR_EXACT_F32', 'DGR_NO_UP', 'DGR_NO_DSPLIT', 'DGR_OS_MB01', 'DGR_OS_MB2', 'DGR_OS_MB3', 'DGR_OS_CK')
LIST_FIELDS = ('rule_ptr', 'tile_ptr', 'tile_desc', 'pair_in', 'out_ptr', 'out_pos')


@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp('fcgf_wide')
    out = {}
    for name, env, args in (('wide', {}, ['repro']), ('os', {'DGR_NO_WIDE3': '1'}, [])):   # a fresh child per variant
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        path = str(d / f'{name}.npz')
        subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'aux', 'fcgf_wide_dump.py'), path] + args, env=e,
                       check=True, timeout=600)
        out[name] = np.load(path)
    return out


@pytest.fixture(scope='module')
def sd():
    from deepglobalregistration_amd import synth
    return synth.synth_state_dict(3, 1, 32, fc.CONV1_KS, fc.SEED)


def read_lists(maps):
    got = {}
    for kind, ts in fc.MAPS:
        raw = {f: maps.raw(kind, ts, f) for f in LIST_FIELDS}
        for f in ('pair_out', 'pair_k', 'in_ptr', 'in_pos'):   # not kept: refused, not returned empty
            raw[f] = maps_ref._try(maps.raw, kind, ts, f)
            assert raw[f] is None, (kind, ts, f)
        for f in ('K', 'n_cap', 'pair_cap'):
            raw[f] = maps.raw(kind, ts, f)
        got[kind, ts] = raw
    return got


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_lists_keep_the_map_contract(case):
    from deepglobalregistration_amd import ops
    o = fc.oracle_of(case)
    maps = ops.Maps(case.coords, 3, fc.CONV1_KS, lean=True, nbr_lists=True)
    got = read_lists(maps)
    for kind, ts in fc.MAPS:
        raw = got[kind, ts]
        assert raw['K'] == 27 and raw['n_cap'] == o.n_cap and raw['pair_cap'] == 27 * o.n_cap
        k, i, out = o.lib_triplets(kind, ts)
        maps_ref.check_rule_map(f'{case.name} {kind}[{ts}]', raw, maps_ref.expected_rule_map(k, i, out, 27, o.n_cap, False))
    # the lists are the tables' pairs, and the other maps of the object stay unbuilt
    for kind, ts in (('same', 1), ('same', 2), ('down', 1), ('down', 2), ('conv1', 1)):
        assert maps_ref._try(maps.raw, kind, ts, 'rule_ptr') is None, (kind, ts)
    nbr = maps.raw('nbr_same', 8, 'nbr')
    assert (nbr >= 0).sum() == got['same', 8]['rule_ptr'][27]
    again = read_lists(ops.Maps(case.coords, 3, fc.CONV1_KS, lean=True, nbr_lists=True))
    for key, raw in got.items():
        for f, a in raw.items():
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, again[key][f]), (key, f)
    with pytest.raises(ValueError):
        ops.Maps(case.coords, 3, fc.CONV1_KS, lean=False, nbr_lists=True)


_MAPS = {}


def sparse_maps(case):
    if case.name not in _MAPS:
        _MAPS[case.name] = oresunet.SparseMaps(case.coords, 3, fc.CONV1_KS)
    return _MAPS[case.name]


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_every_layer_per_element_against_f64(dumps, sd, case):
    fw = Forward(dumps['wide'], case.name + '/', np.ones((len(case.coords), 1), np.float32))
    maps = sparse_maps(case)
    for li, L in enumerate(ref.LAYERS):
        x, _ = fw.value(L['inp'])
        res = fw.value(L['res'])[0] if L['res'] else None
        y64, B, e32 = ref.run_unit(maps, sd, L, x, res, L['name'] == 'final')
        y, how = fw.value(L['out'])
        assert y.shape == y64.shape and np.isfinite(y).all(), (case, L['name'])
        kind = fw.kinds[li]
        truth, extra = y64, 0.0
        if how != 'f32':   # pieces carry the pending ReLU
            assert ref.RELU[L['out']] and how == ('split6' if li in fc.WIDE_LAYERS else 'dense'), (L['name'], how)
            truth = np.maximum(y64, 0)
            extra = 2.0 ** -22 * np.abs(y).max(axis=1, keepdims=True)
        elif ref.RELU[L['out']] and kind.startswith(('sparse_conv_os<', 'sparse_conv_dense_f16x2', 'sparse_conv_up_f16x2')):
            truth = np.maximum(y64, 0)
        c = 1.5 * e32 + ADD['split']
        err = np.abs(y - truth)
        ratio = float((np.maximum(err - extra, 0) / np.maximum(B, 1e-300)).max())
        print(f'{case.name:12s} {li:2d} {L["name"]:16s} {kind:44s} max |y - f64| / B {ratio:.2e}   f32 reference {e32:.2e}   bound {c:.2e}')
        assert (err <= c * B + extra).all(), (case, li, L['name'], kind, ratio, e32, c)
    # the hand-overs of the wide layers: split rows are the split of the f32 rows they stand next to, bit for bit
    for name in ('T4', 'S4', 'T8', 'U4'):
        planes, scale = ref.encode_split6(fw.get(name, 'f32'), ref.RELU[name])
        assert np.array_equal(scale.view(np.uint32), fw.get(name, 'split_scale').view(np.uint32)), (case, name)
        assert np.array_equal(planes, fw.get(name, 'split_planes')), (case, name)
    for name in ('Y4', 'Y8', 'V4'):   # a block's middle tensor exists as split rows only
        assert not fw.has(name, 'f32') and fw.has(name, 'split_planes'), name
    # ... and the row maxima the output-stationary consumers of reduced tensors read (conv4_tr: S8, conv3_tr: CAT4)
    for name in ('S8', 'CAT4'):
        assert np.array_equal(fw.get(name, 'amax'), ref.row_amax_bits(fw.get(name, 'f32'), ref.RELU[name])), (case, name)
    for name in ('Y4', 'S4', 'T8', 'Y8', 'V4'):
        assert f'{name}/amax' in fw.missing, name


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_every_tensor_agrees_with_the_output_stationary_kernel(dumps, case):
    a = Forward(dumps['wide'], case.name + '/', None)
    b = Forward(dumps['os'], case.name + '/', None)
    for name in [L['out'] for L in ref.LAYERS]:
        x, how = a.value(name)
        y, _ = b.value(name)
        if ref.RELU[name]:   # what every reader sees: pieces carry the pending ReLU, the output-stationary kernels store
            x, y = np.maximum(x, 0), np.maximum(y, 0)   # max(x, 0), a reduction stores the signed rows
        assert x.shape == y.shape and np.isfinite(x).all()
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30))
        print(f'{case.name:12s} {name:4s} max |wide - os| / max |os| = {err:.1e}')
        assert err < KERNEL_VS_KERNEL, (case, name, err)


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_forwards_are_reproducible_also_on_a_share(dumps, case):
    assert int(dumps['wide'][case.name + '/again']) == 1, 'two forwards differ'
    assert int(dumps['wide'][case.name + '/share']) == 1, 'the forward on a quarter share differs from the whole GPU'


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_the_wide_kernel_ran_exactly_where_expected(dumps, case):
    kw, ko = dumps['wide'][case.name + '/kinds'].tolist(), dumps['os'][case.name + '/kinds'].tolist()
    assert len(kw) == len(ko) == 23
    want = {7: '<128, 1, 1>', 8: '<128, 1, 1>', 9: '<128, 2, 1>', 10: '<256, 2, 1>', 11: '<256, 2, 1>', 13: '<128, 1, 1>', 14: '<128, 1, 1>'}
    assert set(want) == set(fc.WIDE_LAYERS)
    for li in range(23):
        if li in want:
            assert kw[li] == 'sparse_conv_wide_f16x2' + want[li], (li, kw[li])
            assert ko[li].startswith('sparse_conv_os<'), (li, ko[li])
        else:
            assert 'sparse_conv_wide' not in kw[li] and kw[li] == ko[li], (li, kw[li], ko[li])
    assert not any('sparse_conv_wide' in k for k in ko)
