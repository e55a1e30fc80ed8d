"""GPU: `ops.voxel_mean` (csrc/voxelmean.hip) against its numpy statement (tests/voxel_mean_ref.py), and the layers above
it (`voxel_down_sample`, `compute_overlap_ratio(downsample='mean')`, `DeepGlobalRegistration.fuse_scene`, the scene
harness).

`first`, `coords`, `count`, `sums`, `mean` and `dropped` are compared for EXACT equality: both sides perform the same
correctly rounded float64 operations in the same order (no fused multiply-add on either side) and integer additions,
whose order does not matter.  No tolerance and no excluded case."""
import numpy as np
import pytest
import torch

from voxel_mean_ref import FRAC_BITS, voxel_mean_ref

pytestmark = pytest.mark.gpu
VOXEL = 0.05
KEYS = ('first', 'coords', 'count', 'sums', 'mean')


def _run(x, voxel, off=None, ids=None, T=None, origin=None):
    from deepglobalregistration_amd import ops
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    r = ops.voxel_mean(t.cuda(), voxel, off, ids, T, origin, return_sums=True)
    assert r['xyz'].dtype == torch.float64 and r['coords'].dtype == torch.int32 and r['count'].dtype == torch.int32
    assert r['first'].dtype == torch.int64 and r['sums'].dtype == torch.int64 and r['xyz'].is_cuda
    out = {k: r[k].cpu().numpy() for k in ('first', 'coords', 'count', 'sums')}
    out['mean'], out['dropped'] = r['xyz'].cpu().numpy(), r['dropped']
    return out


def _same(got, want, what=''):
    assert got['dropped'] == want['dropped'], f'{what}: dropped {got["dropped"]}, statement {want["dropped"]}'
    for k in KEYS:
        assert got[k].shape == want[k].shape, f'{what}: {k} has shape {got[k].shape}, statement {want[k].shape}'
        bad = np.nonzero((got[k] != want[k]).reshape(len(got[k]), int(np.prod(got[k].shape[1:]))).any(1))[0]
        assert len(bad) == 0, f'{what}: {k} differs in {len(bad)} voxels, first {bad[0]}: {got[k][bad[0]]} / {want[k][bad[0]]}'


def _check(x, voxel, off=None, ids=None, T=None, origin=None, what=''):
    got = _run(x, voxel, off, ids, T, origin)
    want = voxel_mean_ref(np.asarray(x), voxel, off, ids, T, origin)
    _same(got, want, what)
    return got


def _random_poses(rng, n, deg=180.0, shift=0.5):
    from deepglobalregistration_amd.synth import _random_rotation
    T = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        T[k, :3, :3], T[k, :3, 3] = _random_rotation(rng, deg), rng.uniform(-shift, shift, 3)
    return T


@pytest.fixture(scope='module')
def scene():
    """The four fragments of synth_scene(0, 4, 3000) voxelised at 5 cm (f32; 2780 / 2767 / 2746 / 2746 rows) with the poses
    that take them back into the room, and the numpy statement of the fused scene, computed once."""
    from deepglobalregistration_amd import synth
    from oracle import pipeline as opipe
    clouds, poses, _ = synth.synth_scene(0, 4, 3000)
    frags = [np.asarray(opipe.preprocess(c, VOXEL)[0], np.float32) for c in clouds]
    off = np.cumsum([0] + [len(f) for f in frags])
    x, T = np.concatenate(frags), np.linalg.inv(poses)
    want = voxel_mean_ref(x, VOXEL, off, None, T)
    assert off.tolist() == [0, 2780, 5547, 8293, 11039] and len(want['first']) == 7020 and want['count'].max() == 7
    return dict(clouds=clouds, frags=frags, x=x, off=off, T=T, want=want)


# ---- 1. the fragments of a scene -------------------------------------------------------------------------------------
def test_scene_under_its_poses(scene):
    got = _run(scene['x'], VOXEL, scene['off'], None, scene['T'])
    _same(got, scene['want'], 'ground-truth poses')
    share = float((got['count'] >= 2).mean())
    print(f'V = {len(got["first"])}, {100 * share:.0f} % of the voxels hold >= 2 points, at most {got["count"].max()}')
    assert 0.3 < share < 0.6


@pytest.mark.parametrize('poses', ['identity', 'random', 'none'])
def test_scene_under_other_poses(scene, poses):
    T = {'identity': np.tile(np.eye(4), (4, 1, 1)), 'random': _random_poses(np.random.default_rng(5), 4), 'none': None}[poses]
    got = _check(scene['x'], VOXEL, scene['off'], None, T, what=poses)
    if poses != 'random':
        assert len(got['first']) == 11032
    if poses == 'none':     # no transform at all equals the identity: 1 x + 0 y + 0 z + 0 is exact
        _same(got, voxel_mean_ref(scene['x'], VOXEL, scene['off'], None, np.tile(np.eye(4), (4, 1, 1))), 'none / identity')


def test_subset_and_the_order_of_the_fragment_list(scene):
    x, off, T = scene['x'], scene['off'], scene['T']
    a = _check(x, VOXEL, off, [3, 1], T[[3, 1]], what='reversed')
    b = _check(x, VOXEL, off, [1, 3], T[[1, 3]], what='sorted')
    _same(a, b, 'reversed against sorted')
    assert ((a['first'] >= off[1]) & (a['first'] < off[2]) | (a['first'] >= off[3])).all()
    # a fragment's contribution does not depend on the unselected fragments: fragment 1 alone, out of the bank and as its
    # own array, is the same set of voxels (`first` counts rows of the array it was given)
    alone = _check(x, VOXEL, off, [1], T[[1]], what='one of four')
    own = _check(scene['frags'][1], VOXEL, None, None, T[[1]], what='its own array')
    own['first'] = own['first'] + off[1]
    _same(alone, own, 'alone against its own array')
    mask = _run(x, VOXEL, off, np.array([False, True, False, True]), T[[1, 3]])
    _same(mask, b, 'bool mask')


# ---- 2. a raw cloud in both dtypes -----------------------------------------------------------------------------------
def test_raw_cloud_in_float64_and_float32(scene):
    raw = np.ascontiguousarray(scene['clouds'][0])                 # 3000 raw points, float64
    assert raw.dtype == np.float64
    g64 = _check(raw, 0.1, origin=[0.013, -0.007, 0.021], what='f64')
    g32 = _check(raw.astype(np.float32), 0.1, origin=[0.013, -0.007, 0.021], what='f32')
    assert 2 <= g64['count'].max() <= 8 and g64['count'].sum() == 3000
    # each dtype is quantised as itself: the f32 cast moves points by ~1e-8 m, 1e5 quanta of the sums
    assert g64['sums'].tobytes() != g32['sums'].tobytes()


# ---- 3. lattice known answers by hand --------------------------------------------------------------------------------
def test_lattice_by_hand():
    q = (1 << FRAC_BITS) // 4
    x = np.array([[0.0625, 0.0, 0.1875], [-0.0625, 0.25, -0.25], [0.1875, -0.0, 0.0625], [-0.1875, 0.4375, -0.0625],
                  [0.5, 0.5, 0.5]], np.float32)
    g = _check(x, 0.25, what='origin 0')
    assert g['first'].tolist() == [0, 1, 4] and g['count'].tolist() == [2, 2, 1]
    assert g['coords'].tolist() == [[0, 0, 0], [-1, 1, -1], [2, 2, 2]]
    assert g['sums'].tolist() == [[4 * q, 0, 4 * q], [4 * q, 3 * q, 3 * q], [0, 0, 0]]
    np.testing.assert_array_equal(g['mean'], [[0.125, 0.0, 0.125], [-0.125, 0.34375, -0.15625], [0.5, 0.5, 0.5]])
    g = _check(x[[0, 2]], 0.25, origin=[0.0625, 0.0625, 0.0], what='origin 1/16')
    assert g['coords'].tolist() == [[0, -1, 0]] and g['sums'].tolist() == [[2 * q, 6 * q, 4 * q]]
    np.testing.assert_array_equal(g['mean'], [[0.125, 0.0, 0.125]])


def test_lattice_range_and_dropped_rows():
    one = 1 << FRAC_BITS
    top, bottom = (2.0 ** 31 - 0.5) * 0.25, -2.0 ** 31 * 0.25
    x = np.array([[top, 0, 0], [2.0 ** 31 * 0.25, 0, 0], [bottom, 0, 0], [np.nextafter(bottom, -np.inf), 0, 0],
                  [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.125, 0.125, 0.125], [-1e-30, 0, 0]], np.float64)
    g = _check(x, 0.25, what='f64 range')
    assert g['dropped'] == 5 and g['first'].tolist() == [0, 2, 7, 8]
    assert g['coords'].tolist() == [[2 ** 31 - 1, 0, 0], [-2 ** 31, 0, 0], [0, 0, 0], [-1, 0, 0]]
    assert g['sums'].tolist() == [[one // 2, 0, 0], [0, 0, 0], [one // 2] * 3, [one, 0, 0]]
    np.testing.assert_array_equal(g['mean'], [[top, 0, 0], [bottom, 0, 0], [0.125] * 3, [0.0, 0, 0]])
    kept = _check(x[[0, 2, 7, 8]], 0.25, what='the kept rows alone')
    for k in ('coords', 'count', 'sums', 'mean'):
        np.testing.assert_array_equal(kept[k], g[k])
    none = _check(x[[1, 4]], 0.25, what='every row dropped')
    assert none['dropped'] == 2 and none['mean'].shape == (0, 3)
    # float32 rows with NaN / inf between good ones, under a pose: the dropped rows change nothing else
    rng = np.random.default_rng(2)
    y = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    T = _random_poses(rng, 1)
    clean = _check(y, 0.25, T=T, what='clean')
    y2 = np.insert(y, [0, 17, 17, 300], np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf], [np.nan] * 3], np.float32), 0)
    dirty = _check(y2, 0.25, T=T, what='with non-finite rows')
    assert dirty['dropped'] == 4
    for k in ('coords', 'count', 'sums', 'mean'):
        np.testing.assert_array_equal(dirty[k], clean[k])


def test_dropped_rows_share_the_key_of_a_valid_voxel():
    """A dropped row is stored with the key (0, 0, 0).  Rows 0 .. 299 are NaN; row 300 and a few later rows, in other
    workgroups of the insert and flag kernels, are real points of voxel (0, 0, 0): the voxel's first row is 300 and its
    count leaves the NaN rows out -- unless the shared unique kernels lose the skip of dropped rows."""
    rng = np.random.default_rng(12)
    N, inside = 1500, [300, 301, 555, 700, 1023, 1024, 1499]
    x = rng.uniform(0.3, 0.9, (N, 3))                                # voxels (1..3, 1..3, 1..3) of 25 cm
    x[:300] = np.nan
    x[inside] = rng.uniform(0.01, 0.24, (len(inside), 3))
    for dtype in (np.float64, np.float32):
        g = _check(x.astype(dtype), 0.25, what=f'NaN rows before voxel 0, {np.dtype(dtype).name}')
        assert g['dropped'] == 300 and g['coords'][0].tolist() == [0, 0, 0]
        assert g['first'][0] == 300 and g['count'][0] == len(inside) and g['count'].sum() == N - 300


# ---- 4. shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 2048, 4096, 4097, 16384, 16385])
def test_row_counts_around_the_block_sizes(N):
    """(4096 / 4097: the one-workgroup scan of the flags starts a second round with a carry; 16384 / 16385: the last size of
    that scan and the first of the three-launch one.)"""
    rng = np.random.default_rng(N)
    x = rng.uniform(-0.4, 0.4, (N, 3)).astype(np.float32)           # ~4000 voxels of 5 cm: several points per voxel
    cut = N // 3
    off = [0, N] if cut == 0 else [0, cut, N]
    _check(x, VOXEL, off, None, _random_poses(rng, len(off) - 1, 10.0, 0.05), what=f'N = {N}')
    _check(x.astype(np.float64), VOXEL, what=f'N = {N}, f64, one fragment')


def test_fragments_of_one_row():
    rng = np.random.default_rng(7)
    N = 257
    x = rng.uniform(-0.2, 0.2, (N, 3)).astype(np.float32)
    T = _random_poses(rng, N, 5.0, 0.02)
    _check(x, VOXEL, np.arange(N + 1), None, T, what='257 fragments of one row')
    ids = rng.permutation(N)[:100]
    _check(x, VOXEL, np.arange(N + 1), ids, T[ids], what='100 of them, shuffled')


def test_many_points_in_one_voxel():
    """70 000 points in ONE voxel: every atomic of the call lands on the same four words; the count passes 65 535 and
    the sums 2^56."""
    rng = np.random.default_rng(8)
    x = rng.uniform(0.05, 0.1 - 1e-6, (70000, 3)).astype(np.float32)
    g = _check(x, VOXEL, what='one voxel')
    assert g['count'].tolist() == [70000] and g['coords'].tolist() == [[1, 1, 1]] and g['sums'].min() > 2 ** 54


def test_distinct_voxels_along_one_axis():
    """65 536 points in 65 536 consecutive voxels of one axis: keys that differ in one word (long probe chains)."""
    x = np.zeros((65536, 3), np.float32)
    x[:, 0] = (np.arange(65536) - 30000 + 0.5) * 0.25               # exact in f32
    x = x[np.random.default_rng(9).permutation(65536)]
    g = _check(x, 0.25, what='one axis')
    assert len(g['first']) == 65536 and (g['count'] == 1).all() and g['first'].tolist() == list(range(65536))
    np.testing.assert_array_equal(g['mean'], x.astype(np.float64))


def test_200k_random_points():
    rng = np.random.default_rng(10)
    x = (rng.uniform(0, 1, (200000, 3)) * [4.0, 3.5, 2.6]).astype(np.float32)
    off = np.array([0, 70001, 70002, 150000, 200000])
    g = _check(x, VOXEL, off, None, _random_poses(rng, 4, 3.0, 0.05), what='200 k')
    assert g['count'].sum() == 200000 and g['count'].max() >= 3


# ---- 5. order and reproducibility ------------------------------------------------------------------------------------
def test_runs_are_bitwise_equal_and_permutations_permute_only_first(scene):
    x, off, T = scene['x'], scene['off'], scene['T']
    a, b = _run(x, VOXEL, off, None, T), _run(x, VOXEL, off, None, T)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (np.diff(a['first']) > 0).all()
    # the rows of every fragment permuted (a fragment keeps its pose)
    rng = np.random.default_rng(11)
    perm = np.concatenate([off[f] + rng.permutation(off[f + 1] - off[f]) for f in range(4)])
    c = _check(x[perm], VOXEL, off, None, T, what='permuted rows')
    assert (np.diff(c['first']) > 0).all() and not np.array_equal(c['first'], a['first'])

    def as_set(r):
        rec = np.concatenate((r['coords'].astype(np.int64), r['count'][:, None].astype(np.int64), r['sums'],
                              r['mean'].view(np.int64)), 1)
        return rec[np.lexsort(rec[:, :3].T[::-1])]
    np.testing.assert_array_equal(as_set(a), as_set(c))


# ---- 6. the layers above ---------------------------------------------------------------------------------------------
def test_voxel_down_sample_uses_the_documented_origin(scene):
    from deepglobalregistration_amd.util.pointcloud import voxel_down_sample
    for raw in (scene['clouds'][0], scene['clouds'][1].astype(np.float32)):
        raw = raw.copy()
        raw[5] = np.nan                                             # not a finite point: no part in the bound, dropped
        raw[9, 1] = -np.inf
        finite = raw[np.isfinite(raw).all(1)]
        origin = finite.min(0).astype(np.float64) - 0.5 * VOXEL
        want = voxel_mean_ref(raw, VOXEL, origin=origin)
        got = voxel_down_sample(raw, VOXEL)
        assert got.dtype == torch.float64 and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), want['mean'])
        assert want['coords'].min() == 0 and want['dropped'] == 2
        # every mean lies inside its voxel: at or above the lower face origin + c voxel EXACTLY (c + S / (n 2^40) >= c, and
        # the product and the sum are monotone), below the upper face up to the rounding of that face's own computation
        lo = origin + want['coords'].astype(np.float64) * VOXEL
        assert (got.cpu().numpy() >= lo).all() and (got.cpu().numpy() <= lo + VOXEL + 1e-12).all()
    shifted = voxel_down_sample(scene['clouds'][0], VOXEL, origin=[0.01, 0.02, 0.03])
    np.testing.assert_array_equal(shifted.cpu().numpy(), voxel_mean_ref(scene['clouds'][0], VOXEL, origin=[0.01, 0.02, 0.03])['mean'])


def test_overlap_ratio_on_averaged_clouds():
    from deepglobalregistration_amd import synth
    from deepglobalregistration_amd.util.pointcloud import compute_overlap_ratio, voxel_down_sample
    from deepglobalregistration_amd import ops
    a, b, T = synth.synth_pair(0, 3000)
    mean = compute_overlap_ratio(a, b, T, VOXEL, downsample='mean')
    composed = compute_overlap_ratio(voxel_down_sample(a, VOXEL), voxel_down_sample(b, VOXEL), T, VOXEL, downsample=False)
    assert mean == composed and 0.0 < mean <= 1.0
    # downsample=True is unchanged: the first point of every voxel
    first = compute_overlap_ratio(a, b, T, VOXEL)
    p0, p1 = ops.voxelize(a, VOXEL)[0], ops.voxelize(b, VOXEL)[0]
    assert first == compute_overlap_ratio(a, b, T, VOXEL, downsample=True) == compute_overlap_ratio(p0, p1, T, VOXEL, downsample=False)
    print(f'overlap ratio: first point {first:.4f}, mean {mean:.4f}')


@pytest.fixture(scope='module')
def method_and_bank(scene):
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    dgr = DeepGlobalRegistration.__new__(DeepGlobalRegistration)    # (no network runs in fuse_scene)
    dgr.device, dgr.voxel_size = torch.device('cuda', torch.cuda.current_device()), VOXEL
    n = len(scene['x'])
    bank = FragmentBank.from_tensors(torch.zeros(n, 4, dtype=torch.int32, device='cuda'), torch.from_numpy(scene['x']).cuda(),
                                     torch.zeros(n, 16, device='cuda'), scene['off'])
    return dgr, bank


def test_fuse_scene(scene, method_and_bank):
    from deepglobalregistration_amd import ops
    dgr, bank = method_and_bank
    T, off, want = scene['T'], scene['off'], scene['want']
    fused = dgr.fuse_scene(bank, T)
    direct = ops.voxel_mean(bank.xyz, VOXEL, bank.off, None, T)
    assert torch.equal(fused['xyz'], direct['xyz']) and torch.equal(fused['count'], direct['count']) and fused['dropped'] == 0
    np.testing.assert_array_equal(fused['xyz'].cpu().numpy(), want['mean'])
    np.testing.assert_array_equal(fused['first_fragment'].cpu().numpy(), np.searchsorted(off, want['first'], 'right') - 1)
    lo = want['coords'] * np.float64(VOXEL)                         # every mean lies inside its voxel (origin 0)
    got = fused['xyz'].cpu().numpy()                                # (the lower face exactly: 0 + c voxel, monotone rounding)
    assert (got >= lo).all() and (got <= lo + VOXEL + 1e-12).all()
    two = dgr.fuse_scene(bank, T, min_points=2)
    keep = want['count'] >= 2
    assert 0 < keep.sum() < len(keep)
    np.testing.assert_array_equal(two['xyz'].cpu().numpy(), want['mean'][keep])
    np.testing.assert_array_equal(two['count'].cpu().numpy(), want['count'][keep])
    # a mask excludes the masked fragments; an id list says the same
    part = voxel_mean_ref(scene['x'], VOXEL, off, [0, 2, 3], T[[0, 2, 3]])
    for sel in (np.array([True, False, True, True]), [3, 0, 2]):
        m = dgr.fuse_scene(bank, T, fragments=sel)
        np.testing.assert_array_equal(m['xyz'].cpu().numpy(), part['mean'])
        assert not (m['first_fragment'] == 1).any()
    coarse = dgr.fuse_scene(bank, T, voxel_size=0.2)
    np.testing.assert_array_equal(coarse['xyz'].cpu().numpy(), voxel_mean_ref(scene['x'], 0.2, off, None, T)['mean'])
    # the raw clouds instead of the bank's voxelised points
    raw = dgr.fuse_scene(bank, T, clouds=scene['clouds'])
    raw_off = np.cumsum([0] + [len(c) for c in scene['clouds']])
    raw_want = voxel_mean_ref(np.concatenate(scene['clouds']), VOXEL, raw_off, None, T)
    np.testing.assert_array_equal(raw['xyz'].cpu().numpy(), raw_want['mean'])
    assert int(raw['count'].sum()) == 12000 and raw['xyz'].dtype == torch.float64


def test_scene_mode_writes_the_fused_cloud(scene, method_and_bank, tmp_path):
    from deepglobalregistration_amd.eval import optimize_scenes, read_ply
    dgr, bank = method_and_bank
    T = scene['T']
    recs = [(0, 1), (1, 2), (2, 3)]
    reach = np.array([True, True, True, False])

    class Dataset:
        scenes = ['room']
        def __len__(self): return len(recs)
        def records(self, s): return [(i, j, np.linalg.inv(np.linalg.inv(T[j]) @ T[i])) for i, j in recs]
        def fragment(self, s, f): return scene['clouds'][f]

    class Method:
        use_icp = False
        voxel_size = VOXEL
        def extract_fragments(self, clouds): return bank
        def register_pairs(self, b, pairs, batch_pairs, safeguard, icp):
            return np.stack([np.linalg.inv(T[j]) @ T[i] for i, j in pairs]), np.zeros(3, np.int32), np.zeros((3, 4), np.float32)
        def optimize_scene(self, b, pairs, Tp):
            return {'poses': T, 'reachable': reach, 'kept': np.array([True, True, False]), 'objective_initial': 2.0,
                    'objective_final': 1.0, 'iterations': 3}
        def fuse_scene(self, *a, **k): return dgr.fuse_scene(*a, **k)
    optimize_scenes(Method(), Dataset(), str(tmp_path / 'traj'), out=lambda s: None, fused_dir=str(tmp_path / 'fused'))
    want = voxel_mean_ref(scene['x'], VOXEL, scene['off'], [0, 1, 2], T[:3])
    back = read_ply(str(tmp_path / 'fused' / 'room.ply'))
    assert back.shape == (len(want['first']), 3)
    np.testing.assert_array_equal(back, want['mean'])
    optimize_scenes(Method(), Dataset(), str(tmp_path / 'traj2'), out=lambda s: None, fused_dir=str(tmp_path / 'fused2'),
                    fused_voxel=0.1)
    assert len(read_ply(str(tmp_path / 'fused2' / 'room.ply'))) == len(voxel_mean_ref(scene['x'], 0.1, scene['off'], [0, 1, 2], T[:3])['first'])
