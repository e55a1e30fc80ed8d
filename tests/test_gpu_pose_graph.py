"""GPU: `ops.pose_graph_optimize` (csrc/posegraph.hip) against the float64 numpy solver of tests/posegraph_ref.py (and scipy's
least squares on F* up to 13 nodes), at the smallest shapes at which the kernel can go wrong -- 6 (n - 1) unknowns below, at
and above the Cholesky panel width, the 128-node cap, a reference node that is not 0, duplicate edges, plain least squares,
a residual rotation next to pi --, bitwise reproducibility, batch invariance, and `DeepGlobalRegistration.optimize_scene` on
a synthetic scene with two wrong pairs.

Pose tolerance.  Both solvers stop on flat directions of F*, so their poses agree less well than their objectives.  The
largest pose-entry difference between the numpy solver and the scipy arbiter over ALL graphs of `posegraph_ref.suite_graphs`
(the 128-node one included), measured on the CPU, is 9.9e-9 (per graph: 4e-16 .. 9.9e-9); the kernel is allowed ten times
that against the numpy solver."""
import numpy as np
import pytest
import torch

import posegraph_ref as R
from deepglobalregistration_amd.core import pose_graph as pg

pytestmark = pytest.mark.gpu

POSE_TOL = 10 * 9.9e-9
ARBITER_MAX_NODES = 13

_GRAPHS = R.suite_graphs()
_REF = {}


def _reference(name):
    """The numpy solver's result (and the arbiter's objective for the small graphs), computed once per graph."""
    if name not in _REF:
        g = _GRAPHS[name]
        ref = R.lm_solve(*R.solve_args(g))
        ref['arbiter'] = R.scipy_solve(*R.solve_args(g))['objective_final'] if g['n'] <= ARBITER_MAX_NODES else None
        _REF[name] = ref
    return _REF[name]


def _solve(graphs):
    from deepglobalregistration_amd import ops
    graphs = list(graphs)
    noff = np.cumsum([0] + [g['n'] for g in graphs])
    eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
    cat = lambda k: np.concatenate([g[k] for g in graphs])
    P, line, stats = ops.pose_graph_optimize(noff, eoff, cat('edges'), cat('X'), cat('info'), cat('uncertain'), cat('P_init'),
                                             [(g['mu'], g['reference_node']) for g in graphs])
    return [(P[noff[k]:noff[k + 1]], line[eoff[k]:eoff[k + 1]], stats[k]) for k in range(len(graphs))]


def _fstar(g, P):
    return pg.robust_objective(P, g['edges'], g['X'], g['info'], g['uncertain'], g['mu'])


@pytest.mark.parametrize('name', list(_GRAPHS))
def test_reaches_the_reference_minimum(name):
    g, ref = _GRAPHS[name], _reference(name)
    P, line, stats = _solve([g])[0]
    F, F_init = _fstar(g, P), _fstar(g, g['P_init'])
    dp = np.abs(P - ref['poses']).max()
    print(f'{name}: n={g["n"]} m={len(g["edges"])} F*_init={F_init:.15g} F*_hip={F:.15g} F*_ref={ref["objective_final"]:.15g} '
          f'arbiter={ref["arbiter"]} pose diff={dp:.3e} steps={int(stats[2])} (ref {ref["iterations"]}) converged={int(stats[3])}')
    # 1. the minimum of the reference solver (and of the arbiter), from the same initial poses
    assert F <= ref['objective_final'] * (1 + 1e-9) + 1e-12
    if ref['arbiter'] is not None:
        assert F <= ref['arbiter'] * (1 + 1e-9) + 1e-12
    # 2. never above the start
    assert F <= F_init
    # 3. every planted outlier is below the prune threshold, every true closure at or above it, certain edges at 1
    out, unc = g['outlier'], g['uncertain']
    assert (line[out] < 0.25).all() and (line[~out & unc] >= 0.25).all() and (line[~unc] == 1.0).all()
    # 4. the gauge node is untouched, bit for bit
    r = g['reference_node']
    np.testing.assert_array_equal(P[r].view(np.int64), g['P_init'][r].view(np.int64))
    # 5. the poses of the reference solver
    assert dp <= POSE_TOL
    np.testing.assert_array_equal(P[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (g['n'], 1)))
    # what the call reports about itself
    assert stats[3] == 1 and 1 <= stats[2] <= 100
    assert stats[0] == pytest.approx(F_init, rel=1e-12, abs=1e-20) and stats[1] == pytest.approx(F, rel=1e-12, abs=1e-20)
    np.testing.assert_allclose(line, pg.line_process(pg.edge_chi2(P, g['edges'], g['X'], g['info']), unc, g['mu']), rtol=1e-10)


def test_one_edge_is_solved_exactly():
    g = _GRAPHS['n2_one_edge']
    P, line, stats = _solve([g])[0]
    np.testing.assert_allclose(P[1], P[0] @ pg.rigid_inverse(g['X'][0]), rtol=0, atol=1e-13)
    assert _fstar(g, P) <= 1e-12 and line.tolist() == [1.0]


def test_129_nodes_are_refused_and_the_context_stays_usable():
    from deepglobalregistration_amd import _lib, ops
    g = _GRAPHS['n3_triangle']
    n = 129
    edges = np.stack((np.arange(n - 1), np.arange(1, n)), 1)
    args = ([0, n], [0, n - 1], edges, np.tile(np.eye(4), (n - 1, 1, 1)), np.tile(np.eye(6), (n - 1, 1, 1)), np.zeros(n - 1, bool),
            np.tile(np.eye(4), (n, 1, 1)))
    with pytest.raises(ValueError, match='at most 128'):
        ops.pose_graph_optimize(*args, [(1.0, 0)])
    # the library's own refusal, behind the wrapper's: DGR_EINVAL before any device work
    noff, eoff, ids, X, info, unc, poses, _ = ops.check_pose_graph_args(
        [0, 128], [0, 127], edges[:127], args[3][:127], args[4][:127], args[5][:127], args[6][:128], [(1.0, 0)])
    noff[1], poses = 129, np.ascontiguousarray(args[6].reshape(n, 16))
    out = np.zeros_like(poses)
    prm = (_lib.PgParams * 1)(_lib.PgParams(1.0, 0, 100, 1e-13))
    f64 = lambda a: a.ctypes.data_as(_lib.c_f64p)
    import ctypes as C
    rc = _lib.load().dgr_pose_graph_optimize(_lib.get_ctx('cuda'), 1, noff.ctypes.data_as(_lib.c_i64p), eoff.ctypes.data_as(_lib.c_i64p),
                                             ids.ctypes.data_as(_lib.c_i32p), f64(X), f64(info), unc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             f64(poses), prm, f64(out), f64(np.zeros(127)), f64(np.zeros(4)), None)
    assert rc == _lib.DGR_EINVAL and b'129 nodes' in _lib.load().dgr_last_error()
    P, _, _ = _solve([g])[0]
    assert np.abs(P - _reference('n3_triangle')['poses']).max() <= POSE_TOL


def test_two_runs_agree_bit_for_bit():
    g = _GRAPHS['n12_10_outliers']
    a, b = _solve([g])[0], _solve([g])[0]
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64))


def test_a_graph_does_not_depend_on_the_others_of_the_call():
    names = ['n13', 'n2_one_edge', 'n128_ring_with_chords', 'n5']
    together = _solve([_GRAPHS[k] for k in names])
    for k, got in zip(names, together):
        alone = _solve([_GRAPHS[k]])[0]
        for x, y in zip(got, alone):
            np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64))


def _pose_error(P, P_true):
    """RMS over the fragments of the pose-entry difference after moving both to the gauge of fragment 0."""
    A = pg.rigid_inverse(P[0])[None] @ P
    B = pg.rigid_inverse(P_true[0])[None] @ P_true
    return float(np.sqrt(((A - B)[:, :3] ** 2).sum((1, 2)).mean()))


def test_optimize_scene_prunes_wrong_pairs_and_improves_on_the_spanning_tree():
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    voxel = 0.05
    clouds, poses, pairs = synth.synth_scene(3, 6, n_raw=4000)
    # fragment k -> the frame of fragment 0: x_0 = poses[0] inv(poses[k]) x_k
    P_true = poses[0][None] @ np.linalg.inv(poses)
    xyz = [ops.voxelize(c, voxel)[0] for c in clouds]
    off = np.cumsum([0] + [len(x) for x in xyz])
    rows = int(off[-1])
    bank = FragmentBank.from_tensors(torch.zeros(rows, 4, dtype=torch.int32, device='cuda'), torch.cat(xyz),
                                     torch.zeros(rows, 32, device='cuda'), off)
    dgr = DeepGlobalRegistration.__new__(DeepGlobalRegistration)      # (neither network runs: scoring and the solver only)
    dgr.device, dgr.voxel_size = torch.device('cuda'), voxel
    rng = np.random.default_rng(5)
    ids = [(i, j) for i, j, _ in pairs]
    assert len(ids) >= 9
    T = R.retract(rng.normal(scale=5e-3, size=(len(ids), 6)), np.stack([t for _, _, t in pairs]))
    wrong = [(0, 4), (5, 1)]
    assert not set(wrong) & set(ids) and not {(4, 0), (1, 5)} & set(ids)
    T_wrong = np.stack([R.random_pose(rng, extent=0.5) for _ in wrong])
    all_ids, all_T = ids + wrong, np.concatenate((T, T_wrong))
    is_wrong = np.arange(len(all_ids)) >= len(ids)
    scores = dgr.score_pairs(bank, all_ids, all_T)
    assert (scores['n_corr'][~is_wrong] > 500).all()
    out = dgr.optimize_scene(bank, all_ids, all_T, scores=scores)
    print('kept', out['kept'], 'l', out['line_process'], 'n_corr', scores['n_corr'], 'F*', out['objective_initial'], out['objective_final'],
          'mu', out['mu'], 'steps', out['iterations'])
    assert not out['kept'][is_wrong].any() and out['kept'][~is_wrong].all()
    assert out['reachable'].all() and out['converged'] and out['objective_final'] <= out['objective_initial']
    assert out['poses'].shape == (6, 4, 4) and np.array_equal(out['poses'][0], np.eye(4))
    used = scores['n_corr'] > 0
    assert np.isnan(out['line_process'][~used]).all() and (out['line_process'][used & ~is_wrong] >= 0.25).all()
    assert out['mu'] == pg.default_mu(scores['information'][used], 2 * voxel)
    unc = np.array([abs(i - j) != 1 for i, j in all_ids])
    tree, reached = pg.spanning_tree_poses(6, np.asarray(all_ids)[used], all_T[used], scores['information'][used, 3, 3], 0, unc[used])
    assert reached.all()
    err_tree, err_opt = _pose_error(tree, P_true), _pose_error(out['poses'], P_true)
    print(f'pose error against the ground truth: spanning tree {err_tree:.4e}, optimised {err_opt:.4e}')
    assert err_opt < err_tree
    # scoring inside the call gives the same answer; all-uncertain edges are allowed
    again = dgr.optimize_scene(bank, all_ids, all_T)
    np.testing.assert_array_equal(again['poses'], out['poses'])
    free = dgr.optimize_scene(bank, all_ids, all_T, scores=scores, uncertain=np.ones(len(all_ids), bool))
    assert not free['kept'][is_wrong].any() and free['kept'][~is_wrong].all()
