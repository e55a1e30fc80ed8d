"""GPU: `ops.pose_graph_optimize` (csrc/posegraph.hip) against the float64 numpy solver of tests/posegraph_ref.py (and scipy's
least squares on F* up to 13 nodes), at the smallest shapes at which the kernel can go wrong -- 6 (n - 1) unknowns below, at
and above the Cholesky panel width, the 128-node cap, a reference node that is not 0, duplicate edges, plain least squares,
a residual rotation next to pi --, bitwise reproducibility, batch invariance, and `DeepGlobalRegistration.optimize_scene` on
a synthetic scene with two wrong pairs.

Pose tolerance.  Both solvers stop on flat directions of F*, so their poses agree less well than their objectives.  The
largest pose-entry difference between the numpy solver and the scipy arbiter over ALL graphs of `posegraph_ref.suite_graphs`
(the 128-node one included), measured on the CPU, is 9.9e-9 (per graph: 4e-16 .. 9.9e-9); the kernel is allowed ten times
that against the numpy solver.

Step by step.  Levenberg-Marquardt corrects itself: with a wrong damping rule, a wrong weight or a wrong off-diagonal
block it reaches the same minimum by another road, and the criteria above let it through (tests/test_pose_graph_cpu.py
prints on which graphs).  So the kernel is also stopped after k = 1, 2, 3, 5 accepted steps (`max_iter`) and held to the
numpy solver stopped there (`posegraph_ref.steps_check`): the same step count, the same `converged`, the same poses.
Tolerance of "the same poses": the numpy solver against itself with a second float64 factorisation (eigh + qr for
Cholesky), largest pose-entry difference over k, measured on the CPU per class of graph (`posegraph_ref.step_class`):
    suite  (the graphs up to 20 nodes that start at the chain)        9.4e-15   (21 ulp of an entry in [2, 4))
    far    (far_*, two_components*, isolated_node, rank1_info, pi_*)  6.5e-9    (far_* 5.5e-12, isolated_node and
                                                                                rank1_info 7e-13, pi_* 9e-16; the two
                                                                                two_components graphs 1.2e-9 and 6.5e-9:
                                                                                nothing but the damping holds their
                                                                                second component in place)
    n128   (n128_ring_with_chords)                                    1.0e-13
A class whose maximum is a few ulp is a sample, not a bound: it is floored at 64 ulp of its largest pose entry (the suite
class, whose entries are below 4: 2.8e-14; the other two are above the floor).  The kernel gets ten times the class value -- another summation order and a blocked
factorisation, the margin POSE_TOL has --: 2.8e-13, 6.5e-8, 1.0e-12.  tests/test_pose_graph_cpu.py measures the noise
again and asserts that these constants still bound it.
Measured on the MI355X, largest |P_hip - P_ref| after k steps per class: suite 2.4e-15 (all_certain, k = 3), far 2.5e-9
(two_components_far, k = 5; without the two_components graphs 1.6e-12, rank1_info at k = 5), n128 1.6e-14 (k = 1) -- each
below the CPU noise of its class, with the reference's step count and `converged` at every k on every graph."""
import numpy as np
import pytest
import torch

import posegraph_ref as R
from deepglobalregistration_amd.core import pose_graph as pg

pytestmark = pytest.mark.gpu

POSE_TOL = 10 * 9.9e-9
ARBITER_MAX_NODES = 13
STEP_NOISE = {'suite': 9.4e-15, 'far': 6.5e-9, 'n128': 1.0e-13}      # two float64 factorisations, k steps (the docstring)
STEP_FLOOR = 64 * 2.0 ** -51                                          # 64 ulp of a pose entry in [2, 4)
STEP_TOL = {c: 10 * max(v, STEP_FLOOR) for c, v in STEP_NOISE.items()}

_GRAPHS = R.suite_graphs()
_STEP_GRAPHS = R.step_graphs()
_ALL = {**_GRAPHS, **_STEP_GRAPHS}
_REF = {}
_STEP_REF = {name: {} for name in _ALL}      # name -> {k: the numpy solver stopped after k steps}
_NO_ARBITER = ('rank1_info',)                # its minimum is a manifold: no pose or arbiter comparison (and 20 s of scipy)


def _reference(name):
    """The numpy solver's result (and the arbiter's objective for the small graphs), computed once per graph."""
    if name not in _REF:
        g = _ALL[name]
        ref = R.lm_solve(*R.solve_args(g))
        arbiter = g['n'] <= ARBITER_MAX_NODES and name not in _NO_ARBITER
        ref['arbiter'] = R.scipy_solve(*R.solve_args(g))['objective_final'] if arbiter else None
        _REF[name] = ref
    return _REF[name]


def _solve(graphs, max_iter=None):
    """One call for `graphs`; `max_iter`: None (the default of 100), one limit for all, or one per graph (None in it too)."""
    from deepglobalregistration_amd import ops
    graphs = list(graphs)
    limits = list(max_iter) if isinstance(max_iter, (list, tuple)) else [max_iter] * len(graphs)
    params = [(g['mu'], g['reference_node']) if k is None else (g['mu'], g['reference_node'], k, 1e-13)
              for g, k in zip(graphs, limits)]
    noff = np.cumsum([0] + [g['n'] for g in graphs])
    eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
    cat = lambda k: np.concatenate([g[k] for g in graphs])
    P, line, stats = ops.pose_graph_optimize(noff, eoff, cat('edges'), cat('X'), cat('info'), cat('uncertain'), cat('P_init'),
                                             params)
    return [(P[noff[k]:noff[k + 1]], line[eoff[k]:eoff[k + 1]], stats[k]) for k in range(len(graphs))]


def _fstar(g, P):
    return pg.robust_objective(P, g['edges'], g['X'], g['info'], g['uncertain'], g['mu'])


def _full_run(name):
    """The end-state criteria of a run to convergence; returns (P, line, stats)."""
    g, ref = _ALL[name], _reference(name)
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
    # ... and by the reference's road: its step count, within the one step the stopping test's rounding decides (the
    # numpy solver itself takes 5 or 6 steps on n3_triangle, by the factorisation it uses)
    assert abs(int(stats[2]) - ref['iterations']) <= 1
    assert stats[0] == pytest.approx(F_init, rel=1e-12, abs=1e-20) and stats[1] == pytest.approx(F, rel=1e-12, abs=1e-20)
    np.testing.assert_allclose(line, pg.line_process(pg.edge_chi2(P, g['edges'], g['X'], g['info']), unc, g['mu']), rtol=1e-10)
    return P, line, stats


@pytest.mark.parametrize('name', list(_GRAPHS))
def test_reaches_the_reference_minimum(name):
    _full_run(name)


def _hip_steps(g, k):
    """`ops.pose_graph_optimize` stopped after at most k accepted steps, as `posegraph_ref.steps_check` wants it."""
    P, line, stats = _solve([g], k)[0]
    return {'poses': P, 'line_process': line, 'objective_initial': stats[0], 'objective_final': stats[1],
            'iterations': int(stats[2]), 'converged': int(stats[3]), 'stats': stats}


def _steps(name):
    """`steps_check` of the kernel on one graph, and after every k what the call says about itself."""
    g, tol = _ALL[name], STEP_TOL[R.step_class(name, _ALL[name])]
    rows = R.steps_check(_hip_steps, g, tol=tol, reference=_STEP_REF[name])
    full = _reference(name)['iterations']
    for k, got, ref, dp in rows:
        print(f'{name} [{R.step_class(name, g)}] k={k}: steps {got["iterations"]} (ref {ref["iterations"]}) converged {got["converged"]} '
              f'(ref {int(ref["converged"])}) |P_hip - P_ref| = {dp:.3e} (tol {tol:.2e}) F* {got["objective_final"]:.15g} (ref {ref["objective_final"]:.15g})')
        assert got['stats'][2] == ref['iterations']
        if k < full:
            assert got['stats'][3] == 0
        np.testing.assert_allclose(got['line_process'], pg.line_process(pg.edge_chi2(got['poses'], g['edges'], g['X'], g['info']),
                                                                        g['uncertain'], g['mu']), rtol=1e-10)
        np.testing.assert_array_equal(got['poses'][g['reference_node']].view(np.int64), g['P_init'][g['reference_node']].view(np.int64))
    return rows


@pytest.mark.parametrize('name', list(_ALL))
def test_k_steps_equal_the_reference(name):
    _steps(name)


@pytest.mark.parametrize('name', ['n5', 'two_components_far', 'reference_last'])
def test_max_iter_0_returns_the_start(name):
    g = _ALL[name]
    P, line, stats = _solve([g], 0)[0]
    np.testing.assert_array_equal(P.view(np.int64), g['P_init'].view(np.int64))
    F_init = _fstar(g, g['P_init'])
    assert stats[0] == pytest.approx(F_init, rel=1e-12, abs=1e-20)
    assert stats.tolist() == [stats[0], stats[0], 0.0, 0.0]
    np.testing.assert_allclose(line, pg.line_process(pg.edge_chi2(g['P_init'], g['edges'], g['X'], g['info']), g['uncertain'], g['mu']),
                               rtol=1e-10)


@pytest.mark.parametrize('name,rejections', [('far_n9', 4), ('far_n13', 10)])
def test_far_starts_go_through_the_reject_loop(name, rejections):
    """Starts 1 and 2 rad / m off the chain: the reference rejects trial steps and re-damps (17 factorisations for 13
    steps, 44 for 27), which the graphs that start at the chain never do -- and the kernel ends where it ends."""
    ref = _reference(name)
    print(f'{name}: reference {ref["iterations"]} steps, {ref["factorisations"]} factorisations, {ref["rejections"]} rejected')
    assert ref['rejections'] >= rejections and ref['factorisations'] == ref['iterations'] + ref['rejections']
    _full_run(name)


@pytest.mark.parametrize('name', ['two_components', 'isolated_node'])
def test_nodes_the_reference_node_cannot_reach(name):
    """A second component and a node without an edge: H is singular but for the damping (the edgeless node's rows are
    zero and take lambda * 1).  Step by step and at the end like every other graph; the edgeless node does not move, the
    loose component stays finite, F* does not rise."""
    g = _ALL[name]
    _steps(name)
    P, line, stats = _full_run(name)
    reached = pg.reachable_nodes(g['n'], g['edges'], reference_node=g['reference_node'])
    assert not reached.all() and np.isfinite(P[~reached]).all()
    assert stats[1] <= stats[0] and _fstar(g, P) <= _fstar(g, g['P_init'])
    if name == 'isolated_node':
        assert not np.isin(g['n'] - 1, g['edges'])
        np.testing.assert_array_equal(P[-1].view(np.int64), g['P_init'][-1].view(np.int64))


def test_rank_deficient_information():
    """Lambda = 300 e3 e3^T on every edge: the minimum is a manifold, so no pose comparison at the end (step by step there
    is one: the same road has the same poses); the reference needs 17 factorisations for 10 steps."""
    g, ref = _ALL['rank1_info'], _reference('rank1_info')
    assert ref['rejections'] >= 4
    _steps('rank1_info')
    P, line, stats = _solve([g])[0]
    F = _fstar(g, P)
    print(f'rank1_info: F*_hip={F:.6g} F*_ref={ref["objective_final"]:.6g} steps={int(stats[2])} (ref {ref["iterations"]})')
    assert F <= ref['objective_final'] * (1 + 1e-9) + 1e-12 and np.isfinite(P).all() and stats[3] == 1


def test_600_graphs_in_one_call():
    """More graphs than compute units, small ones and the cap's mixed, every third stopped after two steps: each is its
    solo result bit for bit (per-graph offsets of the normal matrices, the adjacency lists and their pointers)."""
    small = ['n2_one_edge', 'n3_triangle', 'n4', 'n5']
    names = [small[i % 4] for i in range(600)]
    for i in (0, 300, 599):
        names[i] = 'n128_ring_with_chords'
    limits = [2 if i % 3 == 0 else None for i in range(600)]
    together = _solve([_GRAPHS[k] for k in names], limits)
    solo = {}
    for key in sorted(set(zip(names, limits)), key=str):      # five graphs, with and without the limit
        solo[key] = _solve([_GRAPHS[key[0]]], key[1])[0]
    assert len({k for k, _ in solo}) == 5 and len(solo) == 10
    for i, got in enumerate(together):
        for x, y in zip(got, solo[names[i], limits[i]]):
            np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64), err_msg=f'graph {i} ({names[i]}, max_iter {limits[i]})')
    assert {int(together[i][2][2]) for i in range(0, 600, 3)} == {2}


def test_the_callers_last_rows_come_back_and_change_nothing():
    g = _GRAPHS['reference_node_5']
    h = dict(g)
    h['P_init'], h['X'] = g['P_init'].copy(), g['X'].copy()
    h['P_init'][:, 3], h['X'][:, 3] = (1.0, 2.0, 3.0, 4.0), (5.0, 6.0, 7.0, 8.0)
    (P, line, stats), (Q, line_q, stats_q) = _solve([g])[0], _solve([h])[0]
    np.testing.assert_array_equal(Q[:, :3].view(np.int64), P[:, :3].view(np.int64))
    np.testing.assert_array_equal(Q[:, 3].view(np.int64), h['P_init'][:, 3].view(np.int64))
    np.testing.assert_array_equal(line_q.view(np.int64), line.view(np.int64))
    np.testing.assert_array_equal(stats_q.view(np.int64), stats.view(np.int64))


_PI_AXES = ((0.6, -0.48, 0.64), (0.6, -0.64, 0.48), (-0.8, 0.36, 0.48), (-0.6, -0.64, -0.48))
_PI_GAPS = (1e-3, 2e-6, 1.5e-6, 5e-7, 1e-8, 0.0)


def _coupled_information():
    """Lambda of 50 target points well off the origin: a strong rotation-translation block."""
    q = np.random.default_rng(50).uniform((1.0, -3.0, 0.5), (2.5, -1.0, 2.0), size=(50, 3))
    s = np.zeros(11)
    s[0] = len(q)
    s[2:5] = q.sum(0)
    s[5:] = [(q[:, a] * q[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return R.information_from_sums(s)[0]


@pytest.mark.parametrize('axis', _PI_AXES)
def test_rotation_logarithm_next_to_pi_through_the_public_call(axis):
    """Two nodes at the identity, one certain edge, max_iter = 0: stats[0] is chi2 of the kernel's xi for
    E = [exp(a angle) | t].  Against chi2 of the logarithm the case was built from, (a angle, t) -- no log function --, on
    both sides of the switch to the symmetric part and for axes whose largest entry is negative; the coupling block of
    Lambda makes a wrong sign a wrong chi2, not a 1e-6 one.  At angle = pi both signs are logarithms."""
    a = np.array(axis) / np.linalg.norm(axis)
    t, info = np.array([0.3, -0.2, 0.5]), _coupled_information()
    assert np.abs(info[:3, 3:]).max() > 10.0
    chi2 = lambda w: float(np.concatenate((w, t)) @ info @ np.concatenate((w, t)))
    cases = []
    for d in _PI_GAPS:
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R.so3_exp(a * (np.pi - d)), t
        cases.append({'n': 2, 'edges': np.array([[0, 1]]), 'X': pg.rigid_inverse(E)[None], 'info': info[None], 'uncertain': np.zeros(1, bool),
                      'P_init': np.tile(np.eye(4), (2, 1, 1)), 'mu': 1.0, 'reference_node': 0})
    for d, (P, line, stats) in zip(_PI_GAPS, _solve(cases, 0)):
        want = [chi2(a * (np.pi - d))] + ([chi2(-a * (np.pi - d))] if d == 0.0 else [])
        rel = min(abs(stats[0] - w) / w for w in want)
        print(f'axis {axis} d={d:g}: chi2_hip={stats[0]:.15g} chi2 of the true logarithm={want[0]:.15g} rel={rel:.2e} '
              f'(the other sign: {chi2(-a * (np.pi - d)):.15g})')
        assert rel <= 1e-9
        assert stats.tolist() == [stats[0], stats[0], 0.0, 0.0] and line.tolist() == [1.0]


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
