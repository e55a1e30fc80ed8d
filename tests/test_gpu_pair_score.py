"""GPU: the sums of `ops.score_pairs` (csrc/pairscore.hip) against a float64 brute force, the existing radius search, exact
integer-lattice cases, and the layers above (`DeepGlobalRegistration.score_pairs`, `compute_overlap_ratio`).

`n` is compared for EXACT equality and each of the ten floating-point sums under |got - want| <= 2 n 2^-53 sum|term|: both
sides add the SAME n terms in float64 (the kernel fixes the operation order of a term without fused multiply-add and the
brute force of tests/golden/make_golden_gt_match.py follows it; the products q q^T of widened f32 are exact), only in
different orders, and (n - 1) 2^-53 sum|term| bounds the error of either order.  That the two sides pick the same terms
is independent of rounding because every comparison also asserts that no distance of its input lies within 1e-9
(relative) of the radius and no row has its nearest and second-nearest hit within 1e-9 of each other."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
VOXEL = 0.05
U = 2.0 ** -53

_spec = importlib.util.spec_from_file_location('make_golden_gt_match', os.path.join(GOLDEN, 'make_golden_gt_match.py'))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _pose(axis=(1, 2, 3), deg=25.0, t=(0.3, -0.2, 0.1)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(axis, deg), t
    return T


def _random_pose(rng, deg=8.0, shift=0.05):
    return _pose(rng.normal(size=3), rng.uniform(-deg, deg), rng.uniform(-shift, shift, 3))


def _sums_from_sqdist(d2, x1, radius):
    """(sums [11], sum of |term| [11], margin, gap) of one directed pair from its squared-distance matrix [N0,N1]: the
    partner of a row is the smallest (d^2, j) with d^2 < radius^2 (argmin returns the first of equal minima).  margin:
    smallest relative distance of any d^2 to radius^2; gap: smallest relative gap between a row's two nearest hits."""
    r2 = float(radius) * float(radius)
    x1 = np.asarray(x1, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        m = np.where(d2 < r2, d2, np.inf)
    if m.shape[1] == 0:
        return np.zeros(11), np.zeros(11), np.inf, np.inf
    j = m.argmin(1)
    best = m[np.arange(len(m)), j]
    has = np.isfinite(best)
    finite = d2[np.isfinite(d2)]
    margin = float(np.abs(finite - r2).min() / r2) if finite.size else np.inf
    gap = np.inf
    if m.shape[1] > 1:
        two = np.partition(m, 1, axis=1)[:, :2]
        both = np.isfinite(two[:, 1])
        if both.any():
            gap = float(((two[both, 1] - two[both, 0]) / two[both, 1]).min())
    q = x1[j[has]]
    terms = np.column_stack((np.ones(int(has.sum())), best[has], q, q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
                             q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]))
    return terms.sum(0), np.abs(terms).sum(0), margin, gap


def _brute(x0, x1, T, radius):
    return _sums_from_sqdist(mg.sqdist_f64(mg.transformed_f64(x0, T), x1), x1, radius)


def _assert_row(got, want, absum, what=''):
    assert got[0] == want[0], f'{what}: n = {got[0]}, brute force {want[0]}'
    bound = 2 * want[0] * U * absum
    err = np.abs(got - want)
    assert (err <= bound).all(), f'{what}: |got - want| = {err}, bound {bound}'


def _check(got, x0, x1, T, radius, what=''):
    want, absum, margin, gap = _brute(x0, x1, T, radius)
    assert margin > 1e-9, f'{what}: a distance of this input lies at the radius: choose another seed'
    assert gap > 1e-9, f'{what}: a row of this input has its two nearest hits tied: choose another seed'
    _assert_row(got, want, absum, what)
    return want


def _bank(frags):
    frags = [np.asarray(f, np.float32).reshape(-1, 3) for f in frags]
    return np.concatenate(frags), np.cumsum([0] + [len(f) for f in frags])


def _score(frags, ids, Ts, radius):
    from deepglobalregistration_amd import ops
    xyz, off = _bank(frags)
    out = ops.score_pairs(torch.from_numpy(xyz).cuda(), off, np.asarray(ids), np.asarray(Ts, np.float64), radius)
    assert out.dtype == np.float64 and out.shape == (len(ids), 11)
    return out


@pytest.fixture(scope='module')
def synth0():
    """Voxelised synth_pair(0, 3000): ~2.9 k rows per side, ground-truth pose with rotation; the squared-distance
    matrices of the brute force in both directions, computed once."""
    from deepglobalregistration_amd import synth
    from oracle import pipeline as opipe
    a, b, T = synth.synth_pair(0, 3000)
    p0, p1 = opipe.preprocess(a, VOXEL)[0], opipe.preprocess(b, VOXEL)[0]
    assert 2500 < len(p0) < 3200 and 2500 < len(p1) < 3200 and abs(np.trace(T[:3, :3]) - 3) > 0.01
    Ti = np.linalg.inv(T)
    return dict(raw=(a, b), p0=p0, p1=p1, T=T, Ti=Ti, d2_01=mg.sqdist_f64(mg.transformed_f64(p0, T), p1),
                d2_10=mg.sqdist_f64(mg.transformed_f64(p1, Ti), p0))


# ---- 1. brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [0.05, 0.1])
def test_sums_equal_f64_brute_force(synth0, radius):
    s = synth0
    got = _score([s['p0'], s['p1']], [[0, 1], [1, 0]], [s['T'], s['Ti']], radius)
    for k, (d2, tgt) in enumerate(((s['d2_01'], s['p1']), (s['d2_10'], s['p0']))):
        _, margin, gap = mg.pairs_from_sqdist(d2, radius, 1)
        want, absum, margin2, gap2 = _sums_from_sqdist(d2, tgt, radius)
        print(f'r={radius} direction {k}: n = {int(want[0])}, |d2 - r2| / r2 >= {margin:.2e}, nearest / second gap >= '
              f'{min(gap, gap2):.2e}; |got - want| / bound = {np.abs(got[k] - want)[1:] / (2 * want[0] * U * absum)[1:]}')
        assert margin > 1e-9 and margin2 > 1e-9, 'a distance of this input lies at the radius: choose another seed'
        assert gap > 1e-9 and gap2 > 1e-9, 'a row of this input has its two nearest hits tied: choose another seed'
        assert want[0] > 500
        _assert_row(got[k], want, absum, f'direction {k}')


# ---- 2. against the existing kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [0.05, 0.1])
def test_partners_are_the_first_entries_of_radius_pairs_batch(synth0, radius):
    from deepglobalregistration_amd import ops
    s = synth0
    got = _score([s['p0'], s['p1']], [[0, 1], [1, 0]], [s['T'], s['Ti']], radius)
    x0 = np.concatenate((s['p0'], s['p1'])).astype(np.float32)
    x1 = np.concatenate((s['p1'], s['p0'])).astype(np.float32)
    off0 = [0, len(s['p0']), len(s['p0']) + len(s['p1'])]
    off1 = [0, len(s['p1']), len(s['p0']) + len(s['p1'])]
    pairs, pair_off = ops.radius_pairs_batch(x0, off0, x1, off1, np.stack((s['T'], s['Ti'])), radius, K=1)
    pairs = pairs.cpu().numpy()
    for k, tgt in enumerate((s['p1'], s['p0'])):
        own = pairs[pair_off[k]:pair_off[k + 1]]
        assert len(np.unique(own[:, 0])) == len(own)            # K = 1: one entry per source row that has a hit
        assert got[k, 0] == len(own)
        q = np.asarray(tgt, np.float32).astype(np.float64)[own[:, 1]]
        err = np.abs(got[k, 2:5] - q.sum(0))
        assert (err <= 2 * len(own) * U * np.abs(q).sum(0)).all(), err


# ---- 3. exact arithmetic ---------------------------------------------------------------------------------------------------
def _lattice(shift=0.0):
    g = np.arange(5, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + np.float32(shift)


def _exact_sums(q, d2_each):
    q = q.astype(np.float64)
    return np.array([len(q), len(q) * d2_each, *q.sum(0), *[(q[:, a] * q[:, b]).sum()
                                                           for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]])


@pytest.mark.parametrize('shift', [0.0, -7.0])
def test_integer_lattice_pins_the_strict_test_and_the_tie_order(shift):
    """5x5x5 integer lattice against itself: every value is a small dyadic number, so the sums are exact in any order
    and are compared with ==.  Identity, r = 1: every point is its own partner (the six neighbours at distance exactly 1
    fail the strict test anyway).  t = (0.5, 0, 0), r = 0.75: a point with x < 4 lands midway between itself and its
    +x neighbour (d^2 = 0.25 both): the LOWER row index -- itself, x is the slowest axis -- must win, which sum q shows
    (the other choice adds 100 to sum qx); the x = 4 layer has the one partner.  r = 0.5: 0.25 < 0.25 fails."""
    x = _lattice(shift)
    assert (np.diff(x[::25, 0]) > 0).all()                   # x is the slowest axis: the +x neighbour has the higher index
    half = _pose(deg=0.0, t=(0.5, 0, 0))
    got = _score([x], [[0, 0]] * 3, [np.eye(4), half, half], 1.0)[0]
    np.testing.assert_array_equal(got, _exact_sums(x, 0.0))
    assert got[0] == 125 and got[1] == 0
    got = _score([x], [[0, 0]], [half], 0.75)[0]
    np.testing.assert_array_equal(got, _exact_sums(x, 0.25))
    assert got[2] == x[:, 0].astype(np.float64).sum()
    np.testing.assert_array_equal(_score([x], [[0, 0]], [half], 0.5), np.zeros((1, 11)))
    # the mirror image: t = (-0.5, 0, 0) ties a point with its -x neighbour, which now has the LOWER index and wins
    back = _pose(deg=0.0, t=(-0.5, 0, 0))
    partner = x.copy()
    partner[x[:, 0] > x[:, 0].min(), 0] -= 1
    np.testing.assert_array_equal(_score([x], [[0, 0]], [back], 0.75)[0], _exact_sums(partner, 0.25))


# ---- 4. row counts around wave and block edges; a pair does not depend on the call it is in -----------------------------------
def test_row_counts_around_wave_and_block_edges_and_batch_invariance():
    rng = np.random.default_rng(4)
    sizes = [1, 63, 64, 65, 255, 256, 257, 700]
    tgt = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    frags, Ts = [], []
    for n in sizes:
        T = _random_pose(rng)
        pick = rng.permutation(700)[:n]
        src = (tgt[pick].astype(np.float64) - T[:3, 3]) @ T[:3, :3] + rng.normal(scale=0.02, size=(n, 3))
        frags.append(src.astype(np.float32))
        Ts.append(T)
    frags.append(tgt)
    ids = [[k, len(sizes)] for k in range(len(sizes))]
    joint = _score(frags, ids, Ts, 0.1)
    for k, n in enumerate(sizes):
        want = _check(joint[k], frags[k], tgt, Ts[k], 0.1, f'{n} rows')
        assert 0 < want[0] <= n
    assert joint[0, 0] == 1 and joint[-1, 0] > 256
    for k in range(len(sizes)):
        alone = _score(frags, [ids[k]], [Ts[k]], 0.1)
        np.testing.assert_array_equal(alone[0].view(np.int64), joint[k].view(np.int64))
    # ... nor on the order of the pairs or on a pair being there twice
    order = [5, 2, 7, 2, 0]
    mixed = _score(frags, [ids[k] for k in order], [Ts[k] for k in order], 0.1)
    np.testing.assert_array_equal(mixed.view(np.int64), joint[order].view(np.int64))


# ---- 5. one grid per target fragment, reused ----------------------------------------------------------------------------------
def test_every_ordered_pair_of_a_bank_and_the_self_pairs():
    rng = np.random.default_rng(5)
    frags = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for n in (300, 290, 310, 305)]
    ids = [[i, j] for i in range(4) for j in range(4) if i != j] + [[i, i] for i in range(4)]
    Ts = [_random_pose(rng) for _ in range(12)] + [np.eye(4)] * 4
    got = _score(frags, ids, Ts, 0.1)
    for k, (i, j) in enumerate(ids):
        want = _check(got[k], frags[i], frags[j], Ts[k], 0.1, f'pair {i, j}')
        assert want[0] > 50
    for i in range(4):
        assert got[12 + i, 0] == len(frags[i]) and got[12 + i, 1] == 0


# ---- 6. what takes no part -------------------------------------------------------------------------------------------------------
def test_non_finite_rows_take_no_part():
    rng = np.random.default_rng(6)
    x1 = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    x0 = (x1[:200] + rng.normal(scale=0.02, size=(200, 3))).astype(np.float32)
    T = _pose(deg=3.0, t=(0.01, 0, -0.01))
    y0, y1 = x0.copy(), x1.copy()
    bad0, bad1 = [7, 50, 199], [3, 120, 299]
    y0[7, 1], y0[50, 0], y0[199, 2] = np.nan, np.inf, -np.inf
    y1[3, 2], y1[120, 0], y1[299, 1] = np.nan, -np.inf, np.inf
    got = _score([y0, y1], [[0, 1], [1, 0]], [T, np.linalg.inv(T)], 0.1)
    clean = _check(got[0], y0, y1, T, 0.1, 'with the non-finite rows')      # (a NaN distance is no hit in the brute force)
    assert 50 < clean[0] < 198
    # ... and the same as if those rows were not there at all
    _check(got[0], np.delete(x0, bad0, 0), np.delete(x1, bad1, 0), T, 0.1, 'rows removed')
    _check(got[1], np.delete(x1, bad1, 0), np.delete(x0, bad0, 0), np.linalg.inv(T), 0.1, 'rows removed, reverse')
    # a target without a finite row; a source without one; a source a million away
    nan4 = np.full((4, 3), np.nan, np.float32)
    far = _pose(deg=0.0, t=(1e6, 0, 0))
    got = _score([x0, nan4, x1], [[0, 1], [1, 0], [1, 1], [0, 2], [2, 2]], [T, T, np.eye(4), far, far], 0.1)
    np.testing.assert_array_equal(got, np.zeros((5, 11)))
    got = _score([(x0.astype(np.float64) + 1e6).astype(np.float32), x1], [[0, 1], [1, 0]], [np.eye(4)] * 2, 0.1)
    np.testing.assert_array_equal(got, np.zeros((2, 11)))


def test_far_apart_clusters_take_the_cell_doubling_path():
    """A target of two 50-point clusters 1e4 apart along every axis at r = 0.01: 1e6 cells per axis at the first cell
    size, so the cell edge doubles until the grid fits; sources in both clusters, between them and far outside."""
    rng = np.random.default_rng(7)
    a = rng.uniform(-0.05, 0.05, (50, 3))
    x1 = np.concatenate([a, a[::-1] + 1e4]).astype(np.float32)
    x0 = np.concatenate([x1[:50].astype(np.float64) + rng.normal(scale=0.003, size=(50, 3)),
                         x1[50:].astype(np.float64) + rng.normal(scale=0.003, size=(50, 3)),
                         [[5e3, 5e3, 5e3], [-5e4, 0.0, 0.0], [9e4, 9e4, 9e4]]]).astype(np.float32)
    got = _score([x0, x1], [[0, 1]], [np.eye(4)], 0.01)
    want = _check(got[0], x0, x1, np.eye(4), 0.01, 'clusters')
    lo = _brute(x0[:50], x1, np.eye(4), 0.01)[0][0]
    assert 0 < lo < want[0] and want[0] > 20                 # both clusters have partners


# ---- 7. more pairs than a launch takes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [40000, 70000])
def test_many_pairs_in_one_call(P):
    """An 8-fragment bank of 5-point fragments, P directed pairs drawn with a seed, one call.  A launch takes 65535 pairs
    in its y dimension: 70 000 pairs need two launches (40 000, the count this test was specified with, fit into one)."""
    rng = np.random.default_rng(8)
    frags = rng.uniform(0, 0.3, (8, 5, 3)).astype(np.float32)
    radius = 0.12
    ids = rng.integers(0, 8, (P, 2))
    ang = rng.uniform(-0.2, 0.2, P)
    Ts = np.tile(np.eye(4), (P, 1, 1))
    Ts[:, 0, 0], Ts[:, 0, 1], Ts[:, 1, 0], Ts[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    Ts[:, :3, 3] = rng.uniform(-0.05, 0.05, (P, 3))
    got = _score(list(frags), ids, Ts, radius)
    # the brute force of all pairs at once, in the kernel's operation order
    s, t = frags[ids[:, 0]].astype(np.float64), frags[ids[:, 1]].astype(np.float64)         # [P,5,3]
    x, y, z = s[..., 0], s[..., 1], s[..., 2]
    p = np.stack([((Ts[:, r, 0, None] * x + Ts[:, r, 1, None] * y) + Ts[:, r, 2, None] * z) + Ts[:, r, 3, None]
                  for r in range(3)], -1)
    e = p[:, :, None, :] - t[:, None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]             # [P,5,5]
    r2 = radius * radius
    assert np.abs(d2 - r2).min() / r2 > 1e-9
    m = np.where(d2 < r2, d2, np.inf)
    j = m.argmin(2)
    best = np.take_along_axis(m, j[..., None], 2)[..., 0]
    has = np.isfinite(best)
    two = np.sort(m, 2)[..., :2]
    both = np.isfinite(two[..., 1])
    near, second = two[..., 0][both], two[..., 1][both]
    assert (second > 0).all() and ((second - near) / second).min() > 1e-9      # no row has its two nearest hits tied
    q = np.take_along_axis(t, j[..., None], 1)
    terms = np.concatenate((np.ones((P, 5, 1)), best[..., None], q, (q[..., 0] * q[..., 0])[..., None],
                            (q[..., 0] * q[..., 1])[..., None], (q[..., 0] * q[..., 2])[..., None],
                            (q[..., 1] * q[..., 1])[..., None], (q[..., 1] * q[..., 2])[..., None],
                            (q[..., 2] * q[..., 2])[..., None]), -1)
    terms = np.where(has[..., None], terms, 0.0)
    want, absum = terms.sum(1), np.abs(terms).sum(1)
    assert 0.2 < (want[:, 0] > 0).mean() and (want[:, 0] == 0).any() and (want[:, 0] == 5).any()
    np.testing.assert_array_equal(got[:, 0], want[:, 0])
    assert (np.abs(got - want) <= 2 * want[:, :1] * U * absum).all()
    if P > 65535:
        assert got[65535:, 0].sum() > 100                    # the second launch wrote its rows


# ---- 8. reproducible --------------------------------------------------------------------------------------------------------------
def test_two_runs_agree_bit_for_bit(synth0):
    s = synth0
    args = ([s['p0'], s['p1']], [[0, 1], [1, 0], [0, 0]], [s['T'], s['Ti'], _pose(deg=1.0, t=(0.01, 0, 0))], 0.1)
    a, b = _score(*args), _score(*args)
    assert a[:, 0].min() > 500
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


# ---- 9. the layers above -----------------------------------------------------------------------------------------------------------
def test_method_overlap_and_information(synth0):
    from helpers import harness_dgr
    from deepglobalregistration_amd import synth
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    from deepglobalregistration_amd.core.pair_score import information_from_sums
    from deepglobalregistration_amd.util.pointcloud import compute_overlap_ratio
    s = synth0
    ck = synth.synth_checkpoint(seed=0, voxel_size=VOXEL, feat_conv1_kernel_size=7)
    dgr = harness_dgr({'weights': ck}, torch.device('cuda'))
    rng = np.random.default_rng(9)
    extra = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    xyz, off = _bank([s['p0'], s['p1'], extra])

    def bank_on(device):
        return FragmentBank.from_tensors(torch.zeros(len(xyz), 4, dtype=torch.int32, device=device),
                                         torch.from_numpy(xyz).to(device), torch.zeros(len(xyz), 32, device=device), off)
    bank = bank_on('cuda')
    pairs, Ts = [(0, 1), (2, 0)], np.stack((s['T'], _pose(deg=5.0)))
    out = dgr.score_pairs(bank, pairs, Ts)                                   # radius = 2 voxels
    radius = 2 * VOXEL
    fwd = _sums_from_sqdist(s['d2_01'], s['p1'], radius)
    rev = _sums_from_sqdist(s['d2_10'], s['p0'], radius)
    assert min(fwd[2], rev[2]) > 1e-9
    want_overlap = max(fwd[0][0] / len(s['p0']), rev[0][0] / len(s['p1']))
    assert out['n_corr'][0] == fwd[0][0] and out['fitness'][0] == fwd[0][0] / len(s['p0'])
    assert out['fitness_reverse'][0] == rev[0][0] / len(s['p1'])
    assert out['overlap'][0] == want_overlap and 0.1 < want_overlap < 1
    assert abs(out['inlier_rmse'][0] - np.sqrt(fwd[0][1] / fwd[0][0])) < 1e-12
    direct = _score([s['p0'], s['p1'], extra], [[0, 1], [2, 0]], Ts, radius)
    np.testing.assert_array_equal(out['information'], information_from_sums(direct))
    assert out['information'].shape == (2, 6, 6) and out['information'][0, 3, 3] == fwd[0][0]
    fwd2 = _check(direct[1], extra, s['p0'], Ts[1], radius, 'pair (2, 0)')
    assert out['n_corr'][1] == fwd2[0]
    # compute_overlap_ratio on the fragments as they are: the same number (its radius is ONE voxel_size, as in the reference)
    got = compute_overlap_ratio(s['p0'], torch.from_numpy(s['p1']), s['T'], radius, downsample=False)
    assert got == want_overlap
    one = dgr.score_pairs(bank, [(0, 1)], s['T'][None], radius=VOXEL)
    assert compute_overlap_ratio(s['p0'], s['p1'], s['T'], VOXEL, downsample=False) == one['overlap'][0]
    # downsample=True is ops.voxelize (first point of every voxel) in front of the same call
    from deepglobalregistration_amd import ops
    a, b = s['raw']
    down = compute_overlap_ratio(a, b, s['T'], VOXEL)
    assert down == compute_overlap_ratio(ops.voxelize(a, VOXEL)[0], ops.voxelize(b, VOXEL)[0], s['T'], VOXEL, downsample=False)
    assert 0.05 < down < 1
    with pytest.raises(ValueError, match='the bank is on'):
        dgr.score_pairs(bank_on('cpu'), pairs, Ts)
    with pytest.raises(ValueError, match='pair id outside'):
        dgr.score_pairs(bank, [(0, 3)], s['T'][None])
    with pytest.raises(ValueError, match='empty'):
        dgr.score_pairs(bank, [], np.zeros((0, 4, 4)))
    again = dgr.score_pairs(bank, pairs, Ts)                                 # the context is usable after the refusals
    np.testing.assert_array_equal(again['information'], out['information'])
