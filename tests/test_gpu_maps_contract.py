"""GPU: every array of a built maps object against the numpy contract (tests/maps_ref.py), read back raw -- in the
library's own numbering, nothing translated or sorted on the host -- over the shared cases (tests/maps_cases.py), in the
stand-alone build and in the lean build the network forward uses.  Integer work: every comparison is exact."""
import os

import numpy as np
import pytest

import maps_cases as mc
import maps_ref as ref
from oracle import me_semantics as me

pytestmark = pytest.mark.gpu


def _record(case, ks, lean, oracle, fig):
    """the table of profiles/maps_contract.txt: appended to $DGR_MAPS_REPORT/maps_contract.txt when that is named"""
    rep = os.environ.get('DGR_MAPS_REPORT')
    if not rep:
        return
    os.makedirs(rep, exist_ok=True)
    lines = [f'{case.D}d {case.name} ks={ks} {"lean" if lean else "full"}: rows/level '
             + ' '.join(str(fig["level", ts]["rows"]) for ts in ref.LEVELS)
             + '  longest probe chain/level ' + ' '.join(str(fig["level", ts]["longest_probe_chain"]) for ts in ref.LEVELS)]
    for (kind, ts), f in fig.items():
        if kind == 'level':
            continue
        line = f'    {kind}[{ts}]: pairs {f["pairs"]} largest row {f["largest_row"]} largest rule {f["largest_rule"]} tiles {f["tiles"]}'
        if case.D == 6 and kind in ('same', 'down') and oracle.n_cap <= 4096:
            lo, hi = ref.wave_records(oracle, kind, ts)
            region = ref.region_of(kind, ts)
            exact = np.array_equal(lo, hi)
            line += (f'  search waves {len(lo)}, over their region of {region}: '
                     + (f'{int((lo > region).sum())} (exact)' if exact else f'>= {int((lo > region).sum())}, <= {int((hi > region).sum())} (bounds)')
                     + f', most records {int(hi.max())}')
        lines.append(line)
    with open(os.path.join(rep, 'maps_contract.txt'), 'a') as f:
        f.write('\n'.join(lines) + '\n')


def build_and_check(case, ks, lean, only=None):
    from deepglobalregistration_amd import ops
    maps = ops.Maps(case.coords, case.D, ks, lean=lean)
    got = ref.read_all(maps.raw, case.D, ks, lean)
    oracle = mc.oracle_of(case, ks)
    fig = ref.check_maps(got, oracle, lean, only=only)
    _record(case, ks, lean, oracle, fig)
    return maps, got


@pytest.mark.parametrize('p', mc.params(mc.CASES_3D), ids=mc.param_id)
def test_contract_3d(p):
    case, ks, lean = p
    maps, got = build_and_check(case, ks, lean)
    if case.name == 'probe_wrap':
        # the wrap is there in the table the device built: rows that sit below their home slot
        chains, home, slot = ref.probe_chains(case.coords, got['level', 1, 'table'], got['level', 1, 'mask'])
        assert got['level', 1, 'mask'] == 127 and (slot < home).sum() >= 4 and (home >= 126).sum() >= 6
    if not lean:
        # the translating getters agree with the raw arrays (host sort included)
        k, i, o = maps.kernel_map('down', 2)
        ok, oi, oo = mc.oracle_of(case, ks).triplets('down', 2)
        np.testing.assert_array_equal(np.stack([k, i, o]), np.stack([ok, oi, oo]))


@pytest.mark.parametrize('p', mc.params(mc.CASES_6D), ids=mc.param_id)
def test_contract_6d(p):
    case, ks, lean = p
    # (the 28 k rows of `hundreds`: the two maps test_gpu_maps.py compares, under the full contract)
    only = {('same', 1), ('down', 1)} if case.name == 'hundreds' else None
    maps, got = build_and_check(case, ks, lean, only=only)
    o = mc.oracle_of(case, ks)
    for ts in ref.LEVELS:
        np.testing.assert_array_equal(maps.coords(ts), o.coords[ts])      # the getter translates through canon
    if not lean and only is None:
        k, i, out = maps.kernel_map('same', 4)
        np.testing.assert_array_equal(np.stack([k, i, out]), np.stack(o.triplets('same', 4)))


@pytest.mark.parametrize('D,name,ks', [(3, 'rows513', 5), (6, 'replay_sym_fine_perm', 3), (6, 'replay_strided', 3)])
@pytest.mark.parametrize('lean', [False, True], ids=['full', 'lean'])
def test_two_builds_are_identical(D, name, ks, lean):
    from deepglobalregistration_amd import ops
    case = [c for c in (mc.CASES_3D if D == 3 else mc.CASES_6D) if c.name == name][0]
    a = ref.read_all(ops.Maps(case.coords, D, ks, lean=lean).raw, D, ks, lean)
    other = ops.Maps(mc.cloud3(700, 1) if D == 3 else mc.cloud6(700, 1), D, 3)     # other work in between
    b = ref.read_all(ops.Maps(case.coords, D, ks, lean=lean).raw, D, ks, lean)
    del other
    ref.assert_identical(a, b)
    # and the coordinate hash, whose slots depend on which thread claimed one first, serves the same look-ups
    for ts in ref.LEVELS:
        ref.check_hash_table(f'level[{ts}]', mc.oracle_of(case, ks).lib_coords(ts), b['level', ts, 'table'], b['level', ts, 'mask'])


@pytest.mark.parametrize('lean', [False, True], ids=['full', 'lean'])
def test_capacity_overflow_is_reported_and_leaves_the_context_usable(lean):
    from deepglobalregistration_amd import _lib, ops
    with pytest.raises(_lib.DgrError) as e:
        ops.Maps(mc.CASE_OVERFLOW.coords, 6, 3, lean=lean)
    assert e.value.code == _lib.DGR_ENOMEM and 'kernel-map capacity exceeded' in str(e.value)
    build_and_check(mc.CASE_FITS, 3, lean)          # the same lattice with rows removed, straight afterwards
    build_and_check(mc.CASES_6D[2], 3, lean)


def test_raw_refuses_what_it_does_not_know():
    from deepglobalregistration_amd import ops
    m = ops.Maps(mc.CASES_3D[1].coords, 3, 3)
    for kind, ts, field in (('level', 3, 'coords'), ('level', 1, 'nonsense'), ('nonsense', 1, 'coords'), ('down', 8, 'rule_ptr'),
                            ('same', 1, 'in_pos'), ('same', 1, 'in_ptr'), ('nbr_same', 1, 'perm'), ('nbr_up', 8, 'nbr'),
                            ('level', 1, 'canon'), ('conv1', 2, 'rule_ptr')):
        with pytest.raises(ValueError):
            m.raw(kind, ts, field)
    lean6 = ops.Maps(mc.CASES_6D[1].coords, 6, 3, lean=True)
    for kind, ts, field in (('same', 1, 'pair_out'), ('same', 2, 'pair_k'), ('down', 1, 'pair_k'), ('nbr_same', 1, 'nbr')):
        with pytest.raises(ValueError):
            lean6.raw(kind, ts, field)
    assert len(lean6.raw('same', 1, 'pair_k')) == lean6.raw('same', 1, 'rule_ptr')[729]
    with pytest.raises(ValueError):
        lean6.kernel_map('same', 1)                 # the translating getter needs pair_out
    lean3 = ops.Maps(mc.CASES_3D[1].coords, 3, 5, lean=True)
    for kind in ('same', 'conv1', 'down'):
        with pytest.raises(ValueError):
            lean3.raw(kind, 1, 'rule_ptr')


# ---------------------------------------------------------------------------------------------------------------
# voxelisation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_voxelize_points_on_voxel_boundaries(dtype):
    """x = j * voxel for j in [-20, 20]: the quotient x / voxel lands on or next to an integer, where floor() decides"""
    from deepglobalregistration_amd import ops
    voxel = 0.05
    j = np.arange(-20, 21)
    rng = np.random.default_rng(3)
    x = np.stack([j, rng.permutation(j), rng.permutation(j)], axis=1).astype(dtype) * dtype(voxel)
    x = np.concatenate([x, x[::-1] * dtype(1.0)])            # every point twice: duplicates across the input
    want = np.floor(x / dtype(voxel)).astype(np.int32)
    p, c, sel = ops.voxelize(x, voxel, batch_index=1)
    osel = me.first_occurrence_unique(want)
    np.testing.assert_array_equal(sel.cpu().numpy(), osel)
    np.testing.assert_array_equal(c.cpu().numpy()[:, 1:], want[osel])
    assert (c.cpu().numpy()[:, 0] == 1).all()
    np.testing.assert_array_equal(p.cpu().numpy(), x[osel].astype(np.float32))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_voxelize_keeps_the_smallest_row_across_workgroups(dtype):
    """300 points in voxels of their own, then 3000 points falling into five voxels whose first occurrences lie at rows
    >= 300 and whose duplicates are spread over a dozen 256-row workgroups: the survivor is the smallest row index"""
    from deepglobalregistration_amd import ops
    rng = np.random.default_rng(8)
    voxel = 0.05
    own = (np.stack([np.arange(300) + 10, np.zeros(300), np.zeros(300)], 1) + 0.5) * voxel
    five = np.array([[-3, 0, 1], [-3, 0, 2], [4, -7, 0], [0, 0, -1], [-1, -1, -1]])
    which = rng.integers(0, 5, 3000)
    pts = (five[which] + rng.uniform(0.05, 0.95, (3000, 3))) * voxel
    x = np.concatenate([own, pts]).astype(dtype)
    want = np.floor(x / dtype(voxel)).astype(np.int32)
    assert len(np.unique(want[300:], axis=0)) == 5 and len(np.unique(want, axis=0)) == 305
    first = np.array([300 + int(np.argmax(which == v)) for v in range(5)])
    last = np.array([300 + int(np.nonzero(which == v)[0][-1]) for v in range(5)])
    assert (first >= 256).all() and (last // 256 > first // 256 + 8).all()
    _, c, sel = ops.voxelize(x, voxel)
    np.testing.assert_array_equal(sel.cpu().numpy(), np.concatenate([np.arange(300), np.sort(first)]))
    np.testing.assert_array_equal(c.cpu().numpy()[:, 1:], want[sel.cpu().numpy()])


def test_duplicate_rows_in_different_blocks_are_rejected():
    from deepglobalregistration_amd import ops
    for D, cloud in ((3, mc.cloud3), (6, mc.cloud6)):
        coords = cloud(400, 21).copy()
        coords[300] = coords[0]
        for lean in (False, True):
            with pytest.raises(ValueError):
                ops.Maps(coords, D, 3, lean=lean)
