"""CPU-side checks of the scene path: `FragmentBank` validation, how `DeepGlobalRegistration.register_pairs` groups a
pair list and shifts the per-pair hooks (the library call replaced by a recorder), `synth.synth_scene`, and
`eval.evaluate_batched` with a stub method."""
import types

import numpy as np
import pytest
import torch

from deepglobalregistration_amd import ops, synth
from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
from deepglobalregistration_amd.core.fragment_bank import FragmentBank

VOXEL = 0.05


def _bank(sizes=(5, 3, 4), C=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    coords = torch.randint(-50, 50, (n, 4), generator=g, dtype=torch.int32)
    coords[:, 0] = 0
    return (coords, torch.rand(n, 3, generator=g), torch.rand(n, C, generator=g),
            np.concatenate(([0], np.cumsum(sizes))).astype(np.int64))


# ---- FragmentBank.from_tensors --------------------------------------------------------------------------------------
def test_bank_accepts_well_formed_tensors():
    coords, xyz, F, off = _bank()
    bank = FragmentBank.from_tensors(coords, xyz, F, off)
    assert len(bank) == 3 and bank.n_out == 32
    assert bank.rows(1) == slice(5, 8) and bank.rows(-1) == slice(8, 12)
    assert torch.equal(bank.xyz_of(2), xyz[8:12]) and torch.equal(bank.features_of(0), F[:5])
    assert bank.xyz_of(1).data_ptr() == bank.xyz.data_ptr() + 5 * 3 * 4        # a view, not a copy
    assert bank.features_of(1).data_ptr() == bank.F.data_ptr() + 5 * 32 * 4
    assert bank.nbytes == 12 * (16 + 12 + 128) + 4 * 8
    assert FragmentBank.from_tensors(coords, xyz, F, off.tolist()).off.dtype == np.int64
    with pytest.raises(IndexError):
        bank.rows(3)


@pytest.mark.parametrize('case', ['coords_dtype', 'xyz_dtype', 'F_dtype', 'coords_width', 'xyz_width', 'rows',
                                  'non_monotone', 'empty_fragment', 'off_start', 'off_end', 'C24', 'off_float'])
def test_bank_rejects(case):
    coords, xyz, F, off = _bank()
    if case == 'coords_dtype':
        coords = coords.long()
    elif case == 'xyz_dtype':
        xyz = xyz.double()
    elif case == 'F_dtype':
        F = F.half()
    elif case == 'coords_width':
        coords = coords[:, :3]
    elif case == 'xyz_width':
        xyz = torch.cat((xyz, xyz[:, :1]), 1)
    elif case == 'rows':
        F = F[:-1]
    elif case == 'non_monotone':
        off = np.array([0, 8, 5, 12])
    elif case == 'empty_fragment':
        off = np.array([0, 5, 5, 12])
    elif case == 'off_start':
        off = np.array([1, 5, 8, 12])
    elif case == 'off_end':
        off = np.array([0, 5, 8, 11])
    elif case == 'C24':
        F = F[:, :24]
    elif case == 'off_float':
        off = off.astype(np.float64)
    with pytest.raises(ValueError):
        FragmentBank.from_tensors(coords, xyz, F, off)


# ---- register_pairs: grouping and hooks, the library call recorded ----------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, inlier, bank_coords, bank_xyz, bank_F, bank_off, pair_ids, voxel_size, **kw):
        ids = np.array(pair_ids)
        self.calls.append(dict(ids=ids, kw=kw, off=bank_off))
        n = len(ids)
        T = np.tile(np.eye(4), (n, 1, 1))
        T[:, 0, 3] = ids[:, 0] * 100 + ids[:, 1]      # tells the pairs apart in the concatenated result
        return T, ids[:, 0].astype(np.int32), np.repeat(ids[:, 1:2], 4, 1).astype(np.float32)


@pytest.fixture
def method(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(ops, 'register_pairs', rec)
    m = object.__new__(DeepGlobalRegistration)          # no GPU, no library: only what register_pairs reads
    m.device = torch.device('cpu')
    m.fcgf_model = types.SimpleNamespace(out_channels=32)
    m.inlier_model = types.SimpleNamespace(_handle=lambda: 'inlier-handle')
    m.voxel_size, m.clip_weight_thresh, m.inlier_feature_type = VOXEL, 0.05, 'coords'
    m.ransac_max_iteration, m.ransac_seed = 20000, 0
    return m, rec


PAIRS = [(0, 1), (1, 0), (0, 2), (2, 1), (2, 0), (1, 2), (0, 0)]


@pytest.mark.parametrize('batch_pairs, sizes', [(3, [3, 3, 1]), (1, [1] * 7), (7, [7]), (100, [7]), (6, [6, 1])])
def test_grouping_keeps_order(method, batch_pairs, sizes):
    m, rec = method
    bank = FragmentBank.from_tensors(*_bank())
    T, status, stats = m.register_pairs(bank, PAIRS, batch_pairs=batch_pairs, safeguard=True, icp=True)
    assert [len(c['ids']) for c in rec.calls] == sizes
    assert np.concatenate([c['ids'] for c in rec.calls]).tolist() == [list(p) for p in PAIRS]
    assert all(c['ids'].dtype == np.int32 for c in rec.calls)
    assert T.shape == (7, 4, 4) and T.dtype == np.float64
    assert T[:, 0, 3].tolist() == [i * 100 + j for i, j in PAIRS]
    assert status.tolist() == [i for i, _ in PAIRS] and stats[:, 0].tolist() == [j for _, j in PAIRS]
    kw = rec.calls[0]['kw']
    assert kw['safeguard'] is True and kw['use_icp'] is True and kw['skip_refinement'] is False
    assert kw['forced_logit'] is None and kw['override_idx1'] is None
    assert kw['ransac_hypotheses'] == 20000 and kw['break_threshold_ratio'] == 1e-4


@pytest.mark.parametrize('pairs', [[(0, 3)], [(3, 0)], [(0, 1), (-1, 0)], [(0, 1), (1, -1)], [], np.zeros((0, 2), int),
                                   [(0, 1, 2)], [(0.0, 1.0)]])
def test_bad_pair_lists_raise_before_the_library(method, pairs):
    m, rec = method
    bank = FragmentBank.from_tensors(*_bank())
    with pytest.raises(ValueError):
        m.register_pairs(bank, pairs)
    assert rec.calls == []


def test_bank_mismatches_raise_before_the_library(method):
    m, rec = method
    with pytest.raises(ValueError, match='wide'):
        m.register_pairs(FragmentBank.from_tensors(*_bank(C=16)), [(0, 1)])
    m.device = torch.device('cuda')
    with pytest.raises(ValueError, match='is on'):
        m.register_pairs(FragmentBank.from_tensors(*_bank()), [(0, 1)])
    assert rec.calls == []


def test_hooks_become_rows_of_the_group(method):
    """Sizes 5, 3, 4.  Group 1 = pairs (0,1), (2,1): fragment 1 is fragment 1 of both, at rows 0..2 and 3..5 of the
    group's concatenated fragment 1; group 2 = (1,2) alone starts again at 0."""
    m, rec = method
    bank = FragmentBank.from_tensors(*_bank())
    pairs = [(0, 1), (2, 1), (1, 2)]
    ovr = [np.array([2, -1, 0, 1, -1]), torch.tensor([-1, 2, 0, 1]), [3, -1, 0]]
    fl = [np.arange(5.0).reshape(-1, 1), torch.arange(10.0, 14.0), [20.0, 21.0, 22.0]]
    m.register_pairs(bank, pairs, batch_pairs=2, forced_logits=fl, override_idx1=ovr)
    a, b = rec.calls
    assert a['kw']['override_idx1'].dtype == torch.int64
    assert a['kw']['override_idx1'].tolist() == [2, -1, 0, 1, -1, -1, 5, 3, 4]
    assert b['kw']['override_idx1'].tolist() == [3, -1, 0]
    assert a['kw']['forced_logit'].dtype == torch.float32
    assert a['kw']['forced_logit'].tolist() == [0, 1, 2, 3, 4, 10, 11, 12, 13]
    assert b['kw']['forced_logit'].tolist() == [20, 21, 22]


@pytest.mark.parametrize('hook, value', [('override_idx1', [[0] * 4, [0] * 4]), ('override_idx1', [[0] * 5]),
                                         ('override_idx1', [[0, 0, 0, 0, 3], [0] * 4]),
                                         ('forced_logits', [[0.0] * 5, [0.0] * 5])])
def test_bad_hooks_raise(method, hook, value):
    m, rec = method
    bank = FragmentBank.from_tensors(*_bank())
    with pytest.raises(ValueError):
        m.register_pairs(bank, [(0, 1), (2, 1)], **{hook: value})
    assert rec.calls == []


# ---- synth_scene ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    return synth.synth_scene(3, 8, n_raw=6000)


def _near_share(src, dst, radius):
    try:
        from scipy.spatial import cKDTree
        return float((cKDTree(dst).query(src, k=1)[0] <= radius).mean())
    except ImportError:
        near = np.zeros(len(src), bool)
        for a in range(0, len(src), 512):
            d = src[a:a + 512, None, :] - dst[None]
            near[a:a + 512] = (np.einsum('ijk,ijk->ij', d, d) <= radius * radius).any(1)
        return float(near.mean())


def test_synth_scene_is_deterministic(scene):
    clouds, poses, pairs = scene
    clouds2, poses2, pairs2 = synth.synth_scene(3, 8, n_raw=6000)
    assert len(clouds) == 8 and all(c.shape == (6000, 3) and c.dtype == np.float64 for c in clouds)
    assert all(np.array_equal(a, b) for a, b in zip(clouds, clouds2)) and np.array_equal(poses, poses2)
    assert [(i, j) for i, j, _ in pairs] == [(i, j) for i, j, _ in pairs2]
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(pairs, pairs2))
    other = synth.synth_scene(4, 8, n_raw=6000)[0]
    assert not np.array_equal(clouds[0], other[0])


def test_synth_scene_pairs_overlap_under_their_pose(scene):
    clouds, poses, pairs = scene
    assert pairs and all(0 <= i < j < 8 for i, j, _ in pairs)
    for i, j, T in pairs:
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and np.array_equal(T[3], [0, 0, 0, 1])
        share = _near_share(clouds[i] @ T[:3, :3].T + T[:3, 3], clouds[j], 2 * VOXEL)
        assert share >= 0.3, (i, j, share)
    # the fragments are in frames of their own: without the pose nothing lines up
    i, j, _ = pairs[0]
    assert _near_share(clouds[i], clouds[j], 2 * VOXEL) < 0.3


def test_synth_scene_shares_fragments_between_pairs(scene):
    _, _, pairs = scene
    count = np.bincount(np.array([(i, j) for i, j, _ in pairs]).reshape(-1), minlength=8)
    assert count.max() >= 3, count


# ---- evaluate_batched -----------------------------------------------------------------------------------------------
class _StubMethod:
    """Records the calls; 'registers' a pair by looking up the inverse of its pose (fragments are recognised by their
    first coordinate, which the test sets to the fragment's number)."""
    use_icp = True

    def __init__(self, answers):
        self.answers, self.extract_calls, self.register_calls = answers, [], []

    def extract_fragments(self, clouds):
        tags = [int(round(c[0, 0])) for c in clouds]
        self.extract_calls.append(tags)
        return tags

    def register_pairs(self, bank, pairs, batch_pairs=6, **kw):
        self.register_calls.append((list(pairs), batch_pairs, kw))
        T = np.stack([self.answers[(bank[i], bank[j])] for i, j in pairs])
        return T, np.zeros(len(pairs), np.int32), np.zeros((len(pairs), 4), np.float32)

    def register(self, xyz0, xyz1):
        return self.answers[(int(round(xyz0[0, 0])), int(round(xyz1[0, 0])))]


def _write_scene(root, name, records, rng):
    from deepglobalregistration_amd.eval import write_ply, write_trajectory
    (root / name).mkdir()
    (root / f'{name}-evaluation').mkdir()
    for f in sorted({f for i, j, _ in records for f in (i, j)}):
        xyz = rng.random((20, 3))
        xyz[0, 0] = f
        write_ply(str(root / name / f'cloud_bin_{f}.ply'), xyz)
    write_trajectory(str(root / f'{name}-evaluation' / 'gt.log'), [((i, j, 60), T) for i, j, T in records])


def test_evaluate_batched_matches_evaluate(tmp_path):
    from deepglobalregistration_amd.eval import ThreeDMatchTrajectory, evaluate, evaluate_batched
    rng = np.random.default_rng(0)

    def pose():
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = synth._random_rotation(rng), rng.uniform(-1, 1, 3)
        return T
    recs = {'kitchen': [(0, 2, pose()), (0, 5, pose()), (2, 5, pose()), (5, 7, pose())],
            'study': [(1, 3, pose()), (3, 4, pose())]}
    for name, r in recs.items():
        _write_scene(tmp_path, name, r, rng)
    ds = ThreeDMatchTrajectory(str(tmp_path))
    assert ds.scenes == ['kitchen', 'study'] and len(ds) == 6
    assert [(i, j) for i, j, _ in ds.records('kitchen')] == [(0, 2), (0, 5), (2, 5), (5, 7)]
    assert np.array_equal(ds.records('study')[1][2], recs['study'][1][2])
    assert int(round(ds.fragment('kitchen', 5)[0, 0])) == 5 and ds.fragment('study', 4).shape == (20, 3)
    # poses survive the file bit for bit ('%.17g'), so the stub's answers are exact inverses of what the harness inverts
    answers = {(i, j): np.linalg.inv(T) for s in ds.scenes for i, j, T in ds.records(s)}
    stub = _StubMethod(answers)
    lines = []
    stats, scene_means, summary = evaluate_batched(stub, ds, 0.3, 15.0, batch_pairs=4, out=lines.append)
    assert stub.extract_calls == [[0, 2, 5, 7], [1, 3, 4]]          # once per scene, each occurring fragment once
    assert [c[0] for c in stub.register_calls] == [[(0, 1), (0, 2), (1, 2), (2, 3)], [(0, 1), (1, 2)]]
    assert all(c[1] == 4 and c[2] == {'safeguard': True, 'icp': True} for c in stub.register_calls)
    assert stats.shape == (1, 6, 5)
    assert np.array_equal(stats[0, :, 0], np.ones(6)) and np.array_equal(stats[0, :, 1], np.zeros(6))
    # RRE of a rotation against itself is the metric's own zero: rte_rre clips the cosine to 1 - 1e-16 and tr(R^T R) of
    # an orthonormal R carries a few ulps (nine products), so arccos returns sqrt(2 * k * 1.1e-16) rad for a small k:
    # 8.5e-7 deg at k = 1, under 3e-6 deg up to k = 12
    assert (stats[0, :, 2] < 3e-6).all(), stats[0, :, 2]
    assert stats[0, :, 4].tolist() == [0, 0, 0, 0, 1, 1]
    assert (stats[0, :, 3] > 0).all() and len(set(stats[0, :4, 3])) == 1      # a scene's time, shared by its records
    ref_stats, ref_means, ref_summary = evaluate([stub], ['DGR'], ds, 0.3, 15.0, out=lambda s: None)
    assert np.array_equal(stats[:, :, [0, 1, 2, 4]], ref_stats[:, :, [0, 1, 2, 4]])
    assert np.array_equal(scene_means, ref_means) and scene_means.shape == (1, 2, 3)
    assert summary['DGR']['pairs'] == 6 and summary['DGR']['recall'] == ref_summary['DGR']['recall'] == 1.0
    assert len(lines) == 1 and lines[0].startswith('DGR: recall 1.0000 over 6 pairs')
