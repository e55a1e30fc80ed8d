"""GPU: ground-truth matches (fixed-radius pairs), correctness labels, validation counts and `validate_collated`
(csrc/gtmatch.hip) against a float64 brute force, the reference's labels (tests/golden/gt_match.npz) and numpy.

The pair lists are compared for EXACT equality.  That is meaningful because the kernel fixes the operation order of its
float64 arithmetic (no fused multiply-add) and the brute force of tests/golden/make_golden_gt_match.py follows it; and it is
independent of that agreement because the test also asserts that no distance of the input lies within 1e-9 (relative) of
the radius and no K-th / (K+1)-th distance of a capped row within 1e-9 of each other -- float64 rounding is 1e-16."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
VOXEL = 0.05

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


def _gpu_pairs(x0, x1, T, r, K=None):
    from deepglobalregistration_amd import ops
    return ops.radius_pairs(np.asarray(x0, np.float32), np.asarray(x1, np.float32), T, r, K).cpu().numpy()


@pytest.fixture(scope='module')
def synth0():
    """Voxelised synth_pair(0, 3000): ~2.9 k rows per side, ground-truth pose with rotation; the squared-distance matrix
    of the brute force, computed once."""
    from deepglobalregistration_amd import synth
    from oracle import pipeline as opipe
    a, b, T = synth.synth_pair(0, 3000)
    p0, p1 = opipe.preprocess(a, VOXEL)[0], opipe.preprocess(b, VOXEL)[0]
    assert 2500 < len(p0) < 3200 and 2500 < len(p1) < 3200 and abs(np.trace(T[:3, :3]) - 3) > 0.01
    return p0, p1, T, mg.sqdist_f64(mg.transformed_f64(p0, T), p1)


@pytest.mark.parametrize('K', [None, 1, 3])
@pytest.mark.parametrize('radius', [0.05, 0.075, 0.1])
def test_pairs_equal_f64_brute_force(synth0, radius, K):
    p0, p1, T, d2 = synth0
    want, margin, gap = mg.pairs_from_sqdist(d2, radius, K)
    print(f'r={radius} K={K}: {len(want)} pairs, up to {np.bincount(want[:, 0]).max()} per row, '
          f'|d2 - r2| / r2 >= {margin:.2e}, K-th gap >= {gap:.2e}')
    assert margin > 1e-9, 'a distance of this input lies at the radius: choose another seed'
    assert gap > 1e-9, 'a capped row of this input has its K-th and (K+1)-th distance tied: choose another seed'
    assert len(want) > 500
    got = _gpu_pairs(p0, p1, T, radius, K)
    assert got.dtype == np.int64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_get_matching_indices_is_the_same_list(synth0):
    from deepglobalregistration_amd.util.pointcloud import get_matching_indices
    p0, p1, T, d2 = synth0

    class Cloud:                     # an object with .points, like o3d.geometry.PointCloud
        def __init__(self, p):
            self.points = p
    want = mg.pairs_from_sqdist(d2, 2 * VOXEL, 2)[0]
    got = get_matching_indices(Cloud(p0), torch.from_numpy(p1), torch.from_numpy(T), 2 * VOXEL, K=2)
    assert got.is_cuda and got.dtype == torch.int64
    assert got.cpu().tolist() == want.tolist()


def _lattice(shift=0.0):
    g = np.arange(5, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + np.float32(shift)


@pytest.mark.parametrize('shift', [0.0, -7.0])
def test_integer_lattice_pins_strict_test_cell_borders_and_tie_order(shift):
    """5x5x5 integer lattice, identity pose (exact arithmetic).  r = 1: only the point itself -- the six neighbours at
    distance exactly 1 fail the strict test.  r = 1.5: self, 6 at d^2 = 1, 12 at d^2 = 2 for an interior point, each group
    in index order.  A shift to negative coordinates changes nothing."""
    x = _lattice(shift)
    got = _gpu_pairs(x, x, np.eye(4), 1.0)
    np.testing.assert_array_equal(got, np.stack((np.arange(125), np.arange(125)), 1))
    got = _gpu_pairs(x, x, np.eye(4), 1.5)
    np.testing.assert_array_equal(got, mg.brute_radius_pairs(x, x, np.eye(4), 1.5))
    centre = 2 * 25 + 2 * 5 + 2
    js = got[got[:, 0] == centre, 1]
    d2 = ((x[js] - x[centre]) ** 2).sum(1)
    assert d2.tolist() == [0.0] + [1.0] * 6 + [2.0] * 12
    assert js[0] == centre and (np.diff(js[1:7]) > 0).all() and (np.diff(js[7:]) > 0).all()
    assert np.bincount(got[:, 0]).min() == 1 + 3 + 3   # a corner: self, 3 edges, 3 face diagonals


def test_duplicated_target_points_and_cap():
    """300 identical target points: 300 hits per source row in index order (equal distances); K = 5 keeps j = 0..4."""
    x1 = np.tile(np.array([[0.25, -0.5, 1.0]], np.float32), (300, 1))
    x0 = x1[:3] + np.array([[0.01, 0, 0], [0, 0.02, 0], [5.0, 0, 0]], np.float32)
    got = _gpu_pairs(x0, x1, np.eye(4), 0.1)
    want = np.concatenate([np.stack((np.full(300, i), np.arange(300)), 1) for i in (0, 1)])
    np.testing.assert_array_equal(got, want)
    got = _gpu_pairs(x0, x1, np.eye(4), 0.1, K=5)
    np.testing.assert_array_equal(got, np.concatenate([np.stack((np.full(5, i), np.arange(5)), 1) for i in (0, 1)]))


def test_empty_and_single_point_clouds():
    e, one = np.zeros((0, 3), np.float32), np.array([[1.0, 2.0, 3.0]], np.float32)
    assert _gpu_pairs(e, one, np.eye(4), 0.1).shape == (0, 2)
    assert _gpu_pairs(one, e, np.eye(4), 0.1).shape == (0, 2)
    assert _gpu_pairs(e, e, np.eye(4), 0.1).shape == (0, 2)
    assert _gpu_pairs(one, one, np.eye(4), 0.1).tolist() == [[0, 0]]
    assert _gpu_pairs(one, one + np.float32(0.5), np.eye(4), 0.1).shape == (0, 2)


def test_far_apart_clusters_take_the_cell_doubling_path():
    """Two target clusters 2000 apart along every axis at r = 0.01: 2e5 cells per axis at the first cell size, far beyond
    the cell budget, so the cell edge doubles many times; queries in both clusters, between them and far outside."""
    rng = np.random.default_rng(3)
    a = rng.uniform(-0.05, 0.05, (200, 3))
    x1 = np.concatenate([a, a[::-1] + 2000.0]).astype(np.float32)
    x0 = np.concatenate([rng.uniform(-0.05, 0.05, (100, 3)), rng.uniform(-0.05, 0.05, (100, 3)) + 2000.0,
                         [[1000.0, 1000.0, 1000.0], [-5000.0, 0.0, 0.0], [9000.0, 9000.0, 9000.0]]]).astype(np.float32)
    d2 = mg.sqdist_f64(mg.transformed_f64(x0, np.eye(4)), x1)
    want, margin, _ = mg.pairs_from_sqdist(d2, 0.01)
    assert margin > 1e-9 and len(want) > 100 and (want[:, 0] >= 100).any() and (want[:, 0] < 100).any()
    np.testing.assert_array_equal(_gpu_pairs(x0, x1, np.eye(4), 0.01), want)


def test_262145_source_rows_reach_the_carry_of_the_block_scan():
    """The offsets of the source rows are scanned in blocks of 1024 rows and the block sums by ONE workgroup, 256 at a
    time with a carry: 262 145 rows are 257 blocks, the first size with a second round.  Rows 0 .. 262 144 of a 64 x 64 x 65
    integer lattice as two batch entries; entry p's targets are its own rows with row % 3 != p, moved by 1/4 along x and
    shuffled -- at r = 1/2 every source row has its moved self (d = 1/4) or nothing (the next point is 3/4 away), all
    exact under the identity pose, so pairs and pair_off follow from the lattice."""
    from deepglobalregistration_amd import ops
    g = np.arange(65, dtype=np.float32)
    N, cut = 262145, 131072
    x0 = np.stack(np.meshgrid(g[:64], g[:64], g, indexing='ij'), -1).reshape(-1, 3)[:N]
    rng = np.random.default_rng(21)
    x1s, want, off1 = [], [], [0]
    for p, (lo, hi) in enumerate([(0, cut), (cut, N)]):
        rows = lo + np.nonzero(np.arange(lo, hi) % 3 != p)[0]
        perm = rng.permutation(len(rows))                            # target j is source row rows[perm[j]]
        x1s.append(x0[rows[perm]] + np.array([0.25, 0, 0], np.float32))
        want.append(np.stack((rows - lo, np.argsort(perm)), 1))
        off1.append(off1[-1] + len(rows))
    T = np.tile(np.eye(4), (2, 1, 1))
    pairs, pair_off = ops.radius_pairs_batch(x0, [0, cut, N], np.concatenate(x1s), off1, T, 0.5)
    assert pair_off.tolist() == [0, len(want[0]), len(want[0]) + len(want[1])] and len(want[1]) > 80000
    np.testing.assert_array_equal(pairs.cpu().numpy(), np.concatenate(want))


def test_non_finite_rows_take_no_part():
    rng = np.random.default_rng(5)
    x1 = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    x0 = (x1[:200] + rng.normal(scale=0.02, size=(200, 3))).astype(np.float32)
    T = _pose(deg=0.0, t=(0, 0, 0))
    clean = mg.brute_radius_pairs(x0, x1, T, 0.1)
    y0, y1 = x0.copy(), x1.copy()
    y0[7, 1], y0[50, 0], y1[3, 2], y1[120, 0], y1[299, 1] = np.nan, np.inf, np.nan, -np.inf, np.nan
    want = clean[~np.isin(clean[:, 0], [7, 50]) & ~np.isin(clean[:, 1], [3, 120, 299])]
    assert 0 < len(want) < len(clean)
    np.testing.assert_array_equal(mg.brute_radius_pairs(y0, y1, T, 0.1), want)    # (the brute force agrees by itself)
    np.testing.assert_array_equal(_gpu_pairs(y0, y1, T, 0.1), want)
    assert _gpu_pairs(y0, np.full((4, 3), np.nan, np.float32), T, 0.1).shape == (0, 2)   # no finite target point at all


def _batch5():
    rng = np.random.default_rng(9)
    sizes = [(300, 280), (0, 50), (1000, 700), (40, 0), (150, 400)]
    x0s, x1s, Ts = [], [], []
    for p, (n0, n1) in enumerate(sizes):
        T = _pose(axis=(1 + p, 2, 3), deg=10.0 * p, t=(0.1 * p, 0.0, -0.05))
        base = rng.uniform(0, 1, (max(n0, n1), 3))
        x0s.append(base[:n0].astype(np.float32))
        x1s.append((base[:n1] @ T[:3, :3].T + T[:3, 3] + rng.normal(scale=0.01, size=(n1, 3))).astype(np.float32))
        Ts.append(T)
    off0 = np.cumsum([0] + [len(x) for x in x0s])
    off1 = np.cumsum([0] + [len(x) for x in x1s])
    return x0s, x1s, np.stack(Ts), off0, off1


@pytest.mark.parametrize('K', [None, 2])
def test_batch_equals_single_calls_and_is_reproducible(K):
    """Five pairs of unequal sizes, two of them with an empty side, through ONE call: the concatenation of the single
    calls; a second run returns the same bytes."""
    from deepglobalregistration_amd import ops
    x0s, x1s, Ts, off0, off1 = _batch5()
    X0, X1 = torch.from_numpy(np.concatenate(x0s)).cuda(), torch.from_numpy(np.concatenate(x1s)).cuda()
    pairs, pair_off = ops.radius_pairs_batch(X0, off0, X1, off1, Ts, 0.04, K)
    singles = [_gpu_pairs(a, b, T, 0.04, K) for a, b, T in zip(x0s, x1s, Ts)]
    assert pair_off.tolist() == np.cumsum([0] + [len(s) for s in singles]).tolist()
    assert len(singles[0]) > 100 and len(singles[2]) > 100 and len(singles[1]) == 0 and len(singles[3]) == 0
    np.testing.assert_array_equal(pairs.cpu().numpy(), np.concatenate(singles))
    for s, a, b, T in zip(singles, x0s, x1s, Ts):
        np.testing.assert_array_equal(s, mg.brute_radius_pairs(a, b, T, 0.04, K))
    again, again_off = ops.radius_pairs_batch(X0, off0, X1, off1, Ts, 0.04, K)
    assert again.cpu().numpy().tobytes() == pairs.cpu().numpy().tobytes() and again_off.tolist() == pair_off.tolist()


def test_capacity_below_the_total_is_an_error():
    from deepglobalregistration_amd import _lib
    lib = _lib.load()
    x = torch.from_numpy(_lattice()).cuda()
    off = (C.c_int64 * 2)(0, 125)
    T = (C.c_double * 16)(*np.eye(4).reshape(-1))
    counts = torch.empty(125, dtype=torch.int32, device='cuda')
    total = C.c_int64(0)

    def call(pairs, cap):
        return lib.dgr_radius_pairs_batch(_lib.get_ctx('cuda'), _lib.ptr(x), off, _lib.ptr(x), off, 1, T, 1.5, 0,
                                          _lib.ptr(counts), _lib.ptr(pairs), cap, C.byref(total), _lib.stream_ptr())
    assert call(None, 0) == _lib.DGR_OK
    n = total.value
    assert n == int(counts.sum()) == len(mg.brute_radius_pairs(_lattice(), _lattice(), np.eye(4), 1.5))
    pairs = torch.full((n, 2), -1, dtype=torch.int64, device='cuda')
    assert call(pairs, n - 1) == _lib.DGR_EINVAL and b'capacity' in lib.dgr_last_error()
    assert int((pairs != -1).sum()) == 0                      # nothing was written
    with pytest.raises(ValueError, match='capacity'):
        _lib.check(call(pairs, n - 1))
    assert call(pairs, n) == _lib.DGR_OK and int((pairs < 0).sum()) == 0


@pytest.mark.parametrize('case', ['default', 'k3', 'batch3', 'collide'])
def test_labels_equal_the_reference(golden, case):
    from deepglobalregistration_amd.core.correspondence import find_correct_correspondence
    g = golden('gt_match')
    lens = g[f'label_{case}_len_batch']
    pos = [g[f'label_{case}_pos{p}'] for p in range(len(lens))]
    pred = [torch.from_numpy(g[f'label_{case}_pred{p}']) for p in range(len(lens))]
    seed = mg.LABEL_SEED[case]
    got = find_correct_correspondence(pos, pred, hash_seed=seed, len_batch=None if seed is not None else lens.tolist())
    assert got.dtype == bool and got.shape == g[f'label_{case}'].shape
    np.testing.assert_array_equal(got, g[f'label_{case}'])


def test_radius_goldens(golden):
    g = golden('gt_match')
    for K in (None, 2):
        np.testing.assert_array_equal(_gpu_pairs(g['radius_x0'], g['radius_x1'], g['radius_T'], float(g['radius_r']), K),
                                      g[f'radius_pairs_K{K or 0}_restated'])


def test_labels_from_radius_pairs_equal_the_distance_test(synth0):
    """Positive pairs from the radius search at K = None: a predicted pair is labelled correct exactly when d < r."""
    from deepglobalregistration_amd import ops
    p0, p1, T, d2 = synth0
    r = 2 * VOXEL
    pos = ops.radius_pairs(p0, p1, T, r)
    rng = np.random.default_rng(1)
    near = np.argmin(np.where(np.isfinite(d2), d2, np.inf), 1)
    j = np.where(rng.random(len(p0)) < 0.5, near, rng.integers(0, len(p1), len(p0)))
    pred = np.stack((np.arange(len(p0)), j), 1).astype(np.int64)
    want = d2[pred[:, 0], pred[:, 1]] < r * r
    assert 0.1 < want.mean() < 0.9
    got = ops.pairs_isin(pos, [0, len(pos)], torch.from_numpy(pred).cuda(), [0, len(pred)], [max(len(p0), len(p1))])
    assert got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy().astype(bool), want)


def _np_counts(label, w, off, thr=0.5):
    out = np.zeros((len(off) - 1, 6), np.int64)
    for p in range(len(off) - 1):
        lab, pr = label[off[p]:off[p + 1]].astype(bool), w[off[p]:off[p + 1]] > thr
        out[p] = [len(lab), lab.sum(), (pr & lab).sum(), (pr & ~lab).sum(), (~pr & ~lab).sum(), (~pr & lab).sum()]
    return out


@pytest.mark.parametrize('sizes', [[1], [63], [64], [65], [10000], [300, 0, 4097, 64]])
def test_validation_counts_equal_numpy(sizes):
    from deepglobalregistration_amd import ops
    rng = np.random.default_rng(sum(sizes))
    n = sum(sizes)
    label = (rng.random(n) < 0.4).astype(np.uint8)
    w = rng.random(n).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.5                      # at the threshold: not predicted (strict >)
    if n > 10:
        w[3] = np.nan                                 # a NaN weight predicts negative
    off = np.cumsum([0] + sizes)
    lab_d, w_d = torch.from_numpy(label).cuda(), torch.from_numpy(w).cuda()
    got = ops.validation_counts(lab_d, w_d, off)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, _np_counts(label, w, off))
    np.testing.assert_array_equal(ops.validation_counts(lab_d.bool(), w_d.reshape(-1, 1), off, threshold=0.25),
                                  _np_counts(label, w, off, 0.25))
    assert ops.validation_counts(lab_d, w_d, off).tobytes() == got.tobytes()


# ---- validate_collated -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dgr():
    from deepglobalregistration_amd import synth
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    ck = synth.synth_checkpoint(seed=0, voxel_size=VOXEL, feat_conv1_kernel_size=7)
    return DeepGlobalRegistration({'weights': ck, 'clip_weight_thresh': 0.05}, torch.device('cuda'))


def _collate(dgr, clouds):
    x0, c0, x1, c1, lens = [], [], [], [], []
    for p, (a, b) in enumerate(clouds):
        xa, ca, _ = dgr.preprocess(a, batch_index=p)
        xb, cb, _ = dgr.preprocess(b, batch_index=p)
        x0.append(xa.cpu().numpy()); c0.append(ca); x1.append(xb.cpu().numpy()); c1.append(cb)
        lens.append([len(xa), len(xb)])
    return {'pcd0': x0, 'pcd1': x1, 'sinput0_C': torch.cat(c0), 'sinput1_C': torch.cat(c1), 'len_batch': lens}


def _expected(dgr, batch, out, radius, **kw):
    """Every statistic of `validate_collated` from ops.batch_output of the same registration call and numpy."""
    from deepglobalregistration_amd import ops
    eps = np.finfo(float).eps
    dgr.register_collated(batch, skip_refinement=True, **kw)
    idx1 = ops.batch_output('cuda', 'idx1').cpu().numpy()
    w = ops.batch_output('cuda', 'weights').cpu().numpy()
    lens = np.asarray(batch['len_batch'])
    o0, o1 = np.cumsum([0] + list(lens[:, 0])), np.cumsum([0] + list(lens[:, 1]))
    T_gt = np.asarray(batch['T_gt'], np.float64)
    n = len(lens)
    label = np.zeros(len(idx1), bool)
    rte, rre, wsum = np.zeros(n), np.zeros(n), np.zeros(n)
    for p in range(n):
        x0, x1, j = batch['pcd0'][p], batch['pcd1'][p], idx1[o0[p]:o0[p + 1]] - o1[p]
        assert (j >= 0).all() and (j < len(x1)).all()
        d2 = mg.sqdist_f64(mg.transformed_f64(x0, T_gt[p]), x1)
        label[o0[p]:o0[p + 1]] = d2[np.arange(len(x0)), j] < radius * radius
        wp = w[o0[p]:o0[p + 1]]
        R, t = ops.weighted_procrustes(torch.from_numpy(x0).cuda(), torch.from_numpy(x1[j]).cuda(), torch.from_numpy(wp).cuda())
        Rg, tg = T_gt[p, :3, :3].astype(np.float32).astype(np.float64), T_gt[p, :3, 3].astype(np.float32).astype(np.float64)
        rte[p] = np.linalg.norm(t.astype(np.float64) - tg)
        rre[p] = np.degrees(np.arccos(np.clip(((R.astype(np.float64) * Rg).sum() - 1) / 2, -0.999, 0.999)))
        wsum[p] = wp.astype(np.float64).sum()
    counts = _np_counts(label, w, o0)
    np.testing.assert_array_equal(out['counts'], counts)
    tp, fp, tn, fn = (int(v) for v in counts[:, 2:].sum(0))
    precision, recall = tp / (tp + fp + eps), tp / (tp + fn + eps)
    tnr = tn / (tn + fp + eps)
    want = {'hit_ratio': label.sum() / len(label), 'precision': precision, 'recall': recall,
            'f1': 2 * (precision * recall) / (precision + recall + eps), 'tpr': recall, 'tnr': tnr,
            'balanced_accuracy': (recall + tnr) / 2}
    for k, v in want.items():
        assert out[k] == v, (k, out[k], v)
    np.testing.assert_allclose(out['rte'], rte, rtol=1e-12, atol=0)      # (float64 rounding of two summation orders)
    np.testing.assert_allclose(out['rre'], rre, rtol=1e-12, atol=0)
    np.testing.assert_allclose(out['wsum'], wsum, rtol=1e-5)      # (the pipeline sums its f32 weights itself)
    valid = wsum > 10
    assert np.abs(wsum - 10).min() > 0.01
    success = (rte < 0.3) & (rre < 15.0) & valid
    assert out['valid'].tolist() == valid.tolist() and out['success'].tolist() == success.tolist()
    np.testing.assert_allclose([out['regist_rte'], out['regist_rre']], [rte.mean(), rre.mean()], rtol=1e-12, atol=0)
    assert out['succ_rate'] == success.mean()
    return counts, label


def test_validate_collated_equals_numpy(dgr):
    """Two synthetic pairs; half of the overlapping rows carry ground-truth matches, the rest the 1-NN of random-weight
    features (wrong), logits forced to +-4 by a rule that disagrees with correctness on a fifth of the rows: every cell
    of the confusion matrix is populated."""
    from deepglobalregistration_amd import synth
    pairs = [synth.synth_pair(s, n_raw=3000) for s in (0, 1)]
    batch = _collate(dgr, [(a, b) for a, b, _ in pairs])
    batch['T_gt'] = torch.from_numpy(np.stack([T for _, _, T in pairs]))
    ov, fl, off1 = [], [], 0
    for p, (_, _, T) in enumerate(pairs):
        gt = synth.gt_correspondences(batch['pcd0'][p], batch['pcd1'][p], T, VOXEL)
        flip = np.random.default_rng(p).random(len(gt)) < 0.2
        ov.append(np.where(gt >= 0, gt + off1, -1))
        fl.append(np.where((gt >= 0) ^ flip, 4.0, -4.0).astype(np.float32))
        off1 += len(batch['pcd1'][p])
    kw = dict(forced_logits=torch.from_numpy(np.concatenate(fl)).cuda(), override_idx1=torch.from_numpy(np.concatenate(ov)).cuda())
    out = dgr.validate_collated(batch, **kw)
    counts, label = _expected(dgr, batch, out, 2 * VOXEL, **kw)
    assert (counts[:, 2:] > 20).all() and 0.05 < out['hit_ratio'] < 0.95
    assert out['num_pos_pairs'].tolist() == [len(mg.brute_radius_pairs(batch['pcd0'][p], batch['pcd1'][p], pairs[p][2], 2 * VOXEL))
                                             for p in range(2)]
    # the same batch carrying its correspondences, as the reference's data loader provides them, at another radius
    pos = [mg.brute_radius_pairs(batch['pcd0'][p], batch['pcd1'][p], pairs[p][2], 1.5 * VOXEL) for p in range(2)]
    out2 = dgr.validate_collated(dict(batch, correspondences=pos), **kw)
    _expected(dgr, batch, out2, 1.5 * VOXEL, **kw)
    assert out2['num_pos_pairs'].tolist() == [len(q) for q in pos] and out2['num_pos_pairs'].sum() < out['num_pos_pairs'].sum()
    assert out2['counts'][:, 1].sum() <= out['counts'][:, 1].sum()     # (a smaller positive set cannot add hits)
    out3 = dgr.validate_collated(batch, matching_radius=1.5 * VOXEL, **kw)
    np.testing.assert_array_equal(out3['counts'], out2['counts'])
    with pytest.raises(ValueError, match='radius'):
        dgr.validate_collated(batch, matching_radius=0.0, **kw)
    with pytest.raises(ValueError, match='T_gt'):
        dgr.validate_collated(dict(batch, T_gt=np.eye(4)), **kw)


def test_validate_collated_perfect_matches_and_logits(dgr):
    """Fragment 1 = the voxelised fragment 0 moved by the ground-truth pose (voxelised again: every row of fragment 0
    keeps a partner within a voxel diagonal < 2 voxels), matches overridden to the ground truth, logits +-4 by
    correctness: hit ratio, precision and recall are exactly 1."""
    from scipy.spatial import cKDTree
    from deepglobalregistration_amd import synth
    clouds, Ts = [], []
    for s in (0, 1):
        a, _, T = synth.synth_pair(s, n_raw=3000)
        p0 = dgr.preprocess(a)[0].cpu().numpy().astype(np.float64)
        clouds.append((a, p0 @ T[:3, :3].T + T[:3, 3]))
        Ts.append(T)
    batch = _collate(dgr, clouds)
    batch['T_gt'] = np.stack(Ts)
    ov, fl, off1 = [], [], 0
    for p, T in enumerate(Ts):
        x0, x1 = batch['pcd0'][p], batch['pcd1'][p]
        d, j = cKDTree(x1.astype(np.float64)).query(x0.astype(np.float64) @ T[:3, :3].T + T[:3, 3])
        assert d.max() < 1.9 * VOXEL
        ov.append(j + off1)
        fl.append(synth.gt_forced_logits(x0, x1[j], T, VOXEL).reshape(-1))
        off1 += len(x1)
    kw = dict(forced_logits=torch.from_numpy(np.concatenate(fl)).cuda(), override_idx1=torch.from_numpy(np.concatenate(ov)).cuda())
    out = dgr.validate_collated(batch, **kw)
    assert out['hit_ratio'] == 1.0 and out['precision'] == 1.0 and out['recall'] == 1.0 and out['f1'] == 1.0
    assert (out['counts'][:, 0] == out['counts'][:, 2]).all() and out['counts'][:, 3:].sum() == 0
    assert out['succ_rate'] == 1.0 and out['rte'].max() < 0.01
    _expected(dgr, batch, out, 2 * VOXEL, **kw)
