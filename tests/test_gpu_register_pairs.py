"""The scene path on the GPU: `DeepGlobalRegistration.extract_fragments` + `register_pairs` (dgr_register_pairs) against
today's entry points (`preprocess`, `fcgf_feature_extraction`, `register_voxelized`) on the same fragments."""
import numpy as np
import pytest
import torch

from helpers import harness_dgr, rel_err

pytestmark = pytest.mark.gpu
VOXEL = 0.05
F_TOL = 1e-6          # a fragment's features across batch compositions (tests/test_gpu_fullsize.py)
PAIRS = [(0, 1), (1, 0), (0, 2), (4, 1), (2, 4), (3, 0)]


@pytest.fixture(scope='module')
def world():
    """One object, five fragments of one scene (6000, 6000, 3000, 40 and 1500 raw points: fragments 2, 3, 4 are leading
    subsets of their windows' random subsets), voxelised once, and the poses that relate any two of them."""
    from deepglobalregistration_amd import synth
    ck = synth.synth_checkpoint(seed=0, voxel_size=VOXEL, feat_conv1_kernel_size=7)
    dgr = harness_dgr({'weights': ck, 'clip_weight_thresh': 0.05, 'ransac_max_iteration': 20000}, torch.device('cuda'))
    clouds, poses, _ = synth.synth_scene(5, 5, n_raw=6000)
    clouds = [clouds[0], clouds[1], clouds[2][:3000], clouds[3][:40], clouds[4][:1500]]
    vox = [dgr.preprocess(c)[:2] for c in clouds]                   # (xyz, coords), batch column 0
    bank = dgr.extract_fragments(clouds)
    return dict(dgr=dgr, clouds=clouds, poses=poses, vox=vox, bank=bank, cache={})


def _T(world, i, j):
    return world['poses'][j] @ np.linalg.inv(world['poses'][i])


def _concat(world, pairs):
    """The pairs in the layout `register_voxelized` takes: batch column = pair index."""
    c0, x0, c1, x1, off0, off1 = [], [], [], [], [0], [0]
    for p, (i, j) in enumerate(pairs):
        for f, cs, xs, off in ((i, c0, x0, off0), (j, c1, x1, off1)):
            x, c = world['vox'][f]
            c = c.clone()
            c[:, 0] = p
            cs.append(c); xs.append(x); off.append(off[-1] + len(x))
    return torch.cat(c0), torch.cat(x0), off0, torch.cat(c1), torch.cat(x1), off1


def _planted(world, pairs):
    """Per pair: matches for EVERY row of fragment 0 (ground truth where there is one, a seeded row elsewhere: no row is
    left to the feature search) and the logits the ground-truth pose gives them.  Pair-local rows."""
    from deepglobalregistration_amd import synth
    key = tuple(pairs)
    if key not in world['cache']:
        ovr, fl = [], []
        for p, (i, j) in enumerate(pairs):
            xi, xj = world['vox'][i][0].cpu().numpy(), world['vox'][j][0].cpu().numpy()
            gt = synth.gt_correspondences(xi, xj, _T(world, i, j), VOXEL, frac=0.6, seed=p)
            o = np.where(gt >= 0, gt, np.random.default_rng(100 + p).integers(0, len(xj), len(xi)))
            ovr.append(o.astype(np.int64))
            fl.append(synth.gt_forced_logits(xi, xj[o], _T(world, i, j), VOXEL))
        world['cache'][key] = (ovr, fl)
    return world['cache'][key]


def _outputs(dev='cuda'):
    from deepglobalregistration_amd import ops
    return {k: ops.batch_output(dev, k).cpu().numpy() for k in ('idx1', 'logit', 'weights')}


def _reference(world, pairs, forced, **kw):
    """`register_voxelized` on the concatenated pairs, with the planted hooks moved into the batch's numbering."""
    c0, x0, off0, c1, x1, off1 = _concat(world, pairs)
    if forced:
        ovr, fl = _planted(world, pairs)
        kw['override_idx1'] = torch.from_numpy(np.concatenate([o + off1[p] for p, o in enumerate(ovr)])).cuda()
        kw['forced_logits'] = torch.from_numpy(np.concatenate(fl)).cuda()
    return world['dgr'].register_voxelized(c0, x0, off0, c1, x1, off1, **kw), (off0, off1)


# ---- 1. the tail is the same code ---------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['unforced', 'gate_fails', 'planted'])
def test_same_bits_from_the_features_of_register_voxelized(mode):
    """Three pairs of six distinct fragments through `register_voxelized`; a bank made of exactly the features that call
    computed; the same pairs through `register_pairs`: every output equal bit for bit.
      unforced:   nothing forced, safeguard + ICP on.  Measured: the untrained inlier net PASSES the confidence gate on
                  these pairs (status 0 three times), so this case runs refinement + ICP, not the safeguard;
      gate_fails: logits forced to -20 (bench.py's --force-safeguard), safeguard + ICP on: every pair fails the gate,
                  the RANSAC safeguard answers (status 3) and ICP refines -- the branch the first case was meant to reach;
      planted:    ground-truth matches for a share of the rows and the logits the pose gives the final matches: the
                  6000-point pair reaches the refinement (status 0); the sparser pairs plant fewer than the gate's 200
                  inliers and may stay at status 1 -- equal on both paths either way."""
    forced = mode == 'planted'
    from deepglobalregistration_amd import _lib, ops, synth
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    ck = synth.synth_checkpoint(seed=0, voxel_size=VOXEL, feat_conv1_kernel_size=7)
    dgr = harness_dgr({'weights': ck, 'clip_weight_thresh': 0.05, 'ransac_max_iteration': 20000}, torch.device('cuda'))
    raw = [synth.synth_pair(s, n_raw=n) for s, n in ((0, 6000), (1, 3000), (2, 1500))]
    c0, x0, c1, x1, off0, off1 = [], [], [], [], [0], [0]
    for p, (a, b, _) in enumerate(raw):
        xa, ca, _ = dgr.preprocess(a, batch_index=p)
        xb, cb, _ = dgr.preprocess(b, batch_index=p)
        c0.append(ca); x0.append(xa); c1.append(cb); x1.append(xb)
        off0.append(off0[-1] + len(xa)); off1.append(off1[-1] + len(xb))
    C0, X0, C1, X1 = torch.cat(c0), torch.cat(x0), torch.cat(c1), torch.cat(x1)
    kw, hooks = dict(safeguard=True, icp=True), {}
    if forced:
        ovr = [synth.gt_correspondences(x0[p].cpu().numpy(), x1[p].cpu().numpy(), raw[p][2], VOXEL, seed=p) for p in range(3)]
        ov_cat = torch.from_numpy(np.concatenate([np.where(o >= 0, o + off1[p], -1) for p, o in enumerate(ovr)])).cuda()
        dgr.register_voxelized(C0, X0, off0, C1, X1, off1, override_idx1=ov_cat)
        idx1 = ops.batch_output('cuda', 'idx1').cpu().numpy()          # planted rows + the search's for the rest
        fl = [synth.gt_forced_logits(x0[p].cpu().numpy(), X1.cpu().numpy()[idx1[off0[p]:off0[p + 1]]], raw[p][2], VOXEL)
              for p in range(3)]
        kw = dict(override_idx1=ov_cat, forced_logits=torch.from_numpy(np.concatenate(fl)).cuda())
        hooks = dict(override_idx1=ovr, forced_logits=fl)
    if mode == 'gate_fails':
        low = [np.full(off0[p + 1] - off0[p], -20.0, np.float32) for p in range(3)]
        kw['forced_logits'] = torch.from_numpy(np.concatenate(low)).cuda()
        hooks = dict(safeguard=True, icp=True, forced_logits=low)
    elif mode == 'unforced':
        hooks = dict(safeguard=True, icp=True)
    T, status, stats = dgr.register_voxelized(C0, X0, off0, C1, X1, off1, **kw)
    ref = _outputs()
    F0, F1 = ops.batch_output('cuda', 'F0').reshape(-1, 32), ops.batch_output('cuda', 'F1').reshape(-1, 32)
    bank = FragmentBank.from_tensors(torch.cat((C0, C1)), torch.cat((X0, X1)), torch.cat((F0, F1)),
                                     np.concatenate((off0, off0[-1] + np.asarray(off1[1:]))))
    assert len(bank) == 6
    T2, status2, stats2 = dgr.register_pairs(bank, [(0, 3), (1, 4), (2, 5)], batch_pairs=3, **hooks)
    got = _outputs()
    assert np.array_equal(ops.batch_output('cuda', 'F0').reshape(-1, 32).cpu().numpy(), F0.cpu().numpy())
    assert np.array_equal(ops.batch_output('cuda', 'F1').reshape(-1, 32).cpu().numpy(), F1.cpu().numpy())
    for k in ref:
        assert np.array_equal(ref[k], got[k]), k
    assert np.array_equal(T, T2) and np.array_equal(status, status2) and np.array_equal(stats, stats2)
    code = (status & _lib.STATUS_MASK).tolist()
    print(f'{mode}: status {status.tolist()} iterations {stats[:, 0].tolist()}')
    if mode == 'gate_fails':
        assert code == [3, 3, 3], status
        assert not any(np.array_equal(t, np.eye(4)) for t in T)
    elif mode == 'planted':
        assert code[0] == 0 and stats[0, 0] > 0, (status, stats)


# ---- 2. extraction ----------------------------------------------------------------------------------------------------
def test_extraction_does_not_depend_on_the_chunks(world):
    dgr, bank = world['dgr'], world['bank']
    sizes = [len(x) for x, _ in world['vox']]
    assert len(bank) == 5 and np.array_equal(np.diff(bank.off), sizes) and bank.n_out == 32
    assert dgr.feat_timer.diff > 0
    for i, (x, c) in enumerate(world['vox']):                            # = preprocess of each cloud
        assert torch.equal(bank.xyz_of(i), x) and torch.equal(bank.coords_of(i), c)
    # measured 0 across chunkings and against each fragment alone (a fragment's rows never meet another batch index's,
    # and the kernels sum in an order that does not depend on where the rows sit): equality, not the 1e-6 bound that
    # tests/test_gpu_fullsize.py uses for a pair's features across batch compositions
    # chunks (0, 1), (2, 3, 4): the open chunk closes before fragment 2; then every fragment alone
    for chunk_rows in (sizes[0] + sizes[1] + 1, 1):
        other = dgr.extract_fragments(world['clouds'], chunk_rows=chunk_rows)
        assert np.array_equal(other.off, bank.off)
        assert torch.equal(other.coords, bank.coords) and torch.equal(other.xyz, bank.xyz)
        print(f'chunk_rows={chunk_rows}: largest feature difference {float((other.F - bank.F).abs().max()):.3e}')
        assert torch.equal(other.F, bank.F), chunk_rows
    for i, (x, c) in enumerate(world['vox']):
        alone = dgr.fcgf_feature_extraction(torch.ones(len(x), 1, device='cuda'), c)
        print(f'fragment {i} alone: largest feature difference {float((alone - bank.features_of(i)).abs().max()):.3e}')
        assert torch.equal(alone, bank.features_of(i)), i


# ---- 3. shared fragments, both sides, against today's path -----------------------------------------------------------
def test_shared_fragments_forced_match_register_voxelized(world):
    (T, status, stats), _ = _reference(world, PAIRS, forced=True)
    ovr, fl = _planted(world, PAIRS)
    T2, status2, stats2 = world['dgr'].register_pairs(world['bank'], PAIRS, batch_pairs=6, override_idx1=ovr,
                                                      forced_logits=fl)
    print('forced: status', status.tolist(), 'iterations', stats[:, 0].tolist())
    assert np.array_equal(T, T2) and np.array_equal(status, status2) and np.array_equal(stats, stats2)
    assert 0 in status.tolist()          # the planted pairs do reach the refinement


def test_shared_fragments_unforced_match_register_voxelized(world):
    from deepglobalregistration_amd import ops
    _, (off0, off1) = _reference(world, PAIRS, forced=False)
    ref = _outputs()
    rF0, rF1 = (ops.batch_output('cuda', k).reshape(-1, 32).cpu().numpy() for k in ('F0', 'F1'))
    bank = world['bank']
    world['dgr'].register_pairs(bank, PAIRS, batch_pairs=6)
    got = _outputs()
    gF0, gF1 = (ops.batch_output('cuda', k).reshape(-1, 32).cpu().numpy() for k in ('F0', 'F1'))
    bF = bank.F.cpu().numpy()
    mismatches = 0
    for p, (i, j) in enumerate(PAIRS):
        a0, b0, a1, b1 = off0[p], off0[p + 1], off1[p], off1[p + 1]
        assert np.array_equal(gF0[a0:b0], bF[bank.rows(i)]) and np.array_equal(gF1[a1:b1], bF[bank.rows(j)])   # the gather
        dF = max(np.abs(gF0[a0:b0] - rF0[a0:b0]).max(), np.abs(gF1[a1:b1] - rF1[a1:b1]).max())
        assert dF <= F_TOL, (p, dF)
        ia, ib = ref['idx1'][a0:b0] - a1, got['idx1'][a0:b0] - a1
        assert ib.min() >= 0 and ib.max() < b1 - a1
        rows = np.nonzero(ia != ib)[0]
        mismatches += len(rows)
        if len(rows):    # only near-ties may be decided differently: squared distances from the bank's features in float64
            Fi, Fj = bF[bank.rows(i)].astype(np.float64), bF[bank.rows(j)].astype(np.float64)
            da = ((Fi[rows] - Fj[ia[rows]]) ** 2).sum(1)
            db = ((Fi[rows] - Fj[ib[rows]]) ** 2).sum(1)
            assert np.abs(da - db).max() <= 4e-6, (p, len(rows), np.abs(da - db).max())
        else:
            assert rel_err(got['logit'][a0:b0], ref['logit'][a0:b0]) <= 1e-6, p
    print(f'unforced: {mismatches} of {off0[-1]} matches differ between the two paths')


# ---- 4. grouping does not matter ---------------------------------------------------------------------------------------
def test_grouping_does_not_matter(world):
    ovr, fl = _planted(world, PAIRS)
    runs = [world['dgr'].register_pairs(world['bank'], PAIRS, batch_pairs=b, override_idx1=ovr, forced_logits=fl)
            for b in (1, 4, 6)]
    for T, status, stats in runs[1:]:
        assert np.array_equal(T, runs[0][0]) and np.array_equal(status, runs[0][1]) and np.array_equal(stats, runs[0][2])
    assert runs[0][0].shape == (6, 4, 4) and not np.array_equal(runs[0][0][0], runs[0][0][1])


# ---- 5. errors reach the caller before any launch ----------------------------------------------------------------------
def test_errors_come_from_the_library_and_leave_the_context_usable(world):
    from deepglobalregistration_amd import _lib, ops
    dgr, bank = world['dgr'], world['bank']
    inlier = dgr.inlier_model._handle()

    def call(F=bank.F, ids=((0, 1),)):
        return ops.register_pairs(inlier, bank.coords, bank.xyz, F, bank.off, np.array(ids), VOXEL)
    with pytest.raises(_lib.DgrError, match='fragment id 5'):
        call(ids=((0, 1), (5, 0)))
    with pytest.raises(_lib.DgrError, match='fragment id -1'):
        call(ids=((0, -1),))
    with pytest.raises(_lib.DgrError, match='feature width 24'):
        call(F=bank.F[:, :24].contiguous())
    ctx2 = _lib.new_ctx(torch.device('cuda'))
    _lib.use_ctx(ctx2)
    try:
        with pytest.raises(_lib.DgrError, match='another context'):
            call()
    finally:
        _lib.use_ctx(None)
        _lib.load().dgr_ctx_destroy(ctx2)
    T, status, stats = call()
    assert T.shape == (1, 4, 4) and np.isfinite(T).all() and status.shape == (1,)


# ---- 6. the other entry points are left alone -------------------------------------------------------------------------
def test_register_voxelized_around_register_pairs(world):
    (T, status, stats), _ = _reference(world, PAIRS[:1], forced=False, safeguard=True, icp=True)
    first = _outputs()
    world['dgr'].register_pairs(world['bank'], PAIRS, batch_pairs=6)
    (T3, status3, stats3), _ = _reference(world, PAIRS[:1], forced=False, safeguard=True, icp=True)
    third = _outputs()
    assert np.array_equal(T, T3) and np.array_equal(status, status3) and np.array_equal(stats, stats3)
    for k in first:
        assert np.array_equal(first[k], third[k]), k


# ---- 7. harness ------------------------------------------------------------------------------------------------------
def test_evaluate_batched_on_a_written_scene(world, tmp_path):
    from deepglobalregistration_amd import synth
    from deepglobalregistration_amd.eval import (ThreeDMatchTrajectory, evaluate_batched, rte_rre, write_ply,
                                                 write_trajectory)
    dgr = world['dgr']
    clouds, _, pairs = synth.synth_scene(7, 3, n_raw=3000)
    assert [(i, j) for i, j, _ in pairs] == [(0, 1), (1, 2)]
    (tmp_path / 'room').mkdir()
    (tmp_path / 'room-evaluation').mkdir()
    for k, c in enumerate(clouds):
        write_ply(str(tmp_path / 'room' / f'cloud_bin_{k}.ply'), c)
    write_trajectory(str(tmp_path / 'room-evaluation' / 'gt.log'),
                     [((i, j, 3), np.linalg.inv(T)) for i, j, T in pairs])      # a record's pose maps j into i
    ds = ThreeDMatchTrajectory(str(tmp_path))
    assert dgr.use_icp
    stats, scene_means, summary = evaluate_batched(dgr, ds, 0.3, 15.0, batch_pairs=6, out=lambda s: None)
    bank = dgr.extract_fragments([ds.fragment('room', k) for k in range(3)])
    T, _, _ = dgr.register_pairs(bank, [(0, 1), (1, 2)], 6, safeguard=True, icp=True)
    want = np.stack([rte_rre(T[r], np.linalg.inv(pose), 0.3, 15.0) for r, (_, _, pose) in enumerate(ds.records('room'))])
    assert stats.shape == (1, 2, 5) and scene_means.shape == (1, 1, 3)
    assert np.array_equal(stats[0, :, :3], want), (stats, want)
    assert stats[0, :, 4].tolist() == [0, 0] and (stats[0, :, 3] > 0).all()
    assert np.array_equal(scene_means[0, 0], want.mean(0)) and summary['DGR']['pairs'] == 2
