"""CPU-side checks of the pose-graph optimiser (csrc/posegraph.hip, core/pose_graph.py): the C entry point exists, links
from C99 and refuses every bad argument before any device work; the Python wrappers refuse them before any device state
exists; spanning tree, pruning, connectivity and the default mu on hand-made graphs; chi2 against
`eval.metrics.information_rmse`; the analytic Jacobians of the reference solver against central differences; and the
reference solver (tests/posegraph_ref.py: the yardstick of the GPU tests) against scipy's least squares on F*; the k-step
comparison of the GPU tests -- its noise under a second float64 factorisation, the tolerances taken from it, the three
mutants it must reject and the end-state criteria let through --; and the rotation logarithm next to pi for any axis."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import posegraph_ref as R
from conftest import ROOT
from deepglobalregistration_amd.core import pose_graph as pg


def _build_if_missing():
    from deepglobalregistration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_library_exports_the_entry_point():
    import ctypes as C
    from deepglobalregistration_amd import _lib
    _build_if_missing()
    lib = _lib.load()
    assert 'dgr_pose_graph_optimize' in _lib.SIGNATURES
    assert hasattr(lib, 'dgr_pose_graph_optimize')
    assert C.sizeof(_lib.PgParams) == 24         # double, int, int, double


def test_entry_point_links_from_c_and_checks_arguments(tmp_path):
    """A C99 program links dgr_pose_graph_optimize and gets DGR_EINVAL for every bad argument the header lists -- reported
    before any device work, so the program needs no GPU (the context is a dummy non-NULL pointer)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    _build_if_missing()
    lib_dir = os.path.join(ROOT, 'deepglobalregistration_amd', 'lib')
    src = tmp_path / 'pg_abi.c'
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "dgr_hip.h"
#define NN 130
static double big_pose[NN * 16], big_out[NN * 16];
int main(void) {
  int dummy = 0; dgr_ctx *ctx = (dgr_ctx *)&dummy;
  int64_t noff[2] = {0, 3}, eoff[2] = {0, 2}, noff0[2] = {0, 0}, eoff0[2] = {0, 0}, noff1[2] = {1, 3}, noff_big[2] = {0, 129},
          noff_cap[2] = {0, 128};
  int32_t ids[4] = {0, 1, 1, 2}, ids_hi[4] = {0, 1, 1, 3}, ids_neg[4] = {0, -1, 1, 2}, ids_self[4] = {0, 1, 2, 2};
  double X[32], Xnan[32], info[72], info_inf[72], pose[48], pose_nan[48], pose_last[48], out[48], line[2], stats[4];
  uint8_t unc[2] = {0, 1};
  dgr_pg_params p = {1.0, 0, 100, 1e-13}, p_mu0 = p, p_mun = p, p_munan = p, p_ref = p, p_refn = p, p_it = p, p_tol = p;
  int bad = 0, i, k;
  memset(X, 0, sizeof X); memset(info, 0, sizeof info); memset(pose, 0, sizeof pose);
  for (k = 0; k < 2; ++k) for (i = 0; i < 4; ++i) X[16 * k + 5 * i] = 1.0;
  for (k = 0; k < 3; ++k) for (i = 0; i < 4; ++i) pose[16 * k + 5 * i] = 1.0;
  for (k = 0; k < 2; ++k) for (i = 0; i < 6; ++i) info[36 * k + 7 * i] = 1.0;
  for (k = 0; k < NN; ++k) for (i = 0; i < 16; ++i) big_pose[16 * k + i] = (i % 5 == 0) ? 1.0 : 0.0;
  memcpy(Xnan, X, sizeof X); memcpy(info_inf, info, sizeof info);
  memcpy(pose_nan, pose, sizeof pose); memcpy(pose_last, pose, sizeof pose);
  Xnan[16 + 7] = NAN; info_inf[36 + 3] = INFINITY; pose_nan[32 + 1] = NAN; pose_last[12] = NAN;
  p_mu0.mu = 0.0; p_mun.mu = -1.0; p_munan.mu = NAN; p_ref.reference_node = 3; p_refn.reference_node = -1;
  p_it.max_iter = -1; p_tol.rel_tol = -1.0;
  if (DGR_PG_MAX_NODES != 128) bad += 1;
#define CALL(c, n, no, eo, id, x, in, u, po, pr, o, l, s) \
  bad += dgr_pose_graph_optimize(c, n, no, eo, id, x, in, u, po, pr, o, l, s, 0) != DGR_EINVAL
  CALL(0, 1, noff, eoff, ids, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, 0, eoff, ids, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, 0, ids, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, 0, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, 0, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, 0, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, 0, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, 0, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, 0, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p, 0, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p, out, 0, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p, out, line, 0);
  CALL(ctx, 0, noff, eoff, ids, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, -2, noff, eoff, ids, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff0, eoff, ids, X, info, unc, pose, &p, out, line, stats);      /* an empty graph: no nodes */
  CALL(ctx, 1, noff, eoff0, ids, X, info, unc, pose, &p, out, line, stats);      /* ... no edges */
  CALL(ctx, 1, noff1, eoff, ids, X, info, unc, pose, &p, out, line, stats);      /* offsets start at 0 */
  CALL(ctx, 1, noff, eoff, ids_hi, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids_neg, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids_self, X, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, Xnan, info, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info_inf, unc, pose, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose_nan, &p, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_mu0, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_mun, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_munan, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_ref, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_refn, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_it, out, line, stats);
  CALL(ctx, 1, noff, eoff, ids, X, info, unc, pose, &p_tol, out, line, stats);
  CALL(ctx, 1, noff_big, eoff, ids, X, info, unc, big_pose, &p, big_out, line, stats);   /* 129 nodes */
  /* 128 nodes pass the cap, and the last row of a pose is ignored: these calls WOULD reach the device, so they are made
     with an edge id outside the graph -- the only error left is that id */
  CALL(ctx, 1, noff_cap, eoff, ids_neg, X, info, unc, big_pose, &p, big_out, line, stats);
  CALL(ctx, 1, noff, eoff, ids_hi, X, info, unc, pose_last, &p, out, line, stats);
  printf("%d %s\n", bad, dgr_last_error());
  return bad;
}
''')
    exe = tmp_path / 'pg_abi'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    str(src), '-o', str(exe), '-L', lib_dir, '-ldgr_hip', f'-Wl,-rpath,{lib_dir}',
                    '-Wl,-rpath,/opt/rocm/lib', '-lm'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'edge (1, 3) outside' in out.stdout      # the last call got past the pose check


def _tiny():
    I4, I6 = np.tile(np.eye(4), (3, 1, 1)), np.tile(np.eye(6), (2, 1, 1))
    return dict(node_off=[0, 3], edge_off=[0, 2], edge_ids=[[0, 1], [1, 2]], edge_T=I4[:2], edge_info=I6,
                edge_uncertain=[False, True], pose_init=I4, params=[(1.0, 0)])


def test_wrappers_reject_bad_arguments_before_any_device_state(monkeypatch):
    import torch
    from deepglobalregistration_amd import _lib, ops
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank

    def no_device(*a, **k):
        raise AssertionError('device state touched before the argument check')
    monkeypatch.setattr(_lib, 'load', no_device)
    monkeypatch.setattr(ops, 'get_ctx', no_device)
    monkeypatch.setattr(ops, '_xyz_dev', no_device)
    ok = ops.check_pose_graph_args(**_tiny())
    assert ok[2].dtype == np.int32 and ok[3].shape == (2, 16) and ok[4].shape == (2, 36) and ok[5].dtype == np.uint8
    assert ok[7] == [(1.0, 0, 100, 1e-13)]
    nan4, inf6, nanp = np.tile(np.eye(4), (2, 1, 1)), np.tile(np.eye(6), (2, 1, 1)), np.tile(np.eye(4), (3, 1, 1))
    nan4[1, 0, 3], inf6[0, 2, 2], nanp[2, 1, 1] = np.nan, np.inf, np.nan
    big = dict(_tiny(), node_off=[0, 129], pose_init=np.tile(np.eye(4), (129, 1, 1)))
    cases = [
        (dict(node_off=[0, 0]), 'without nodes or edges'), (dict(edge_off=[0, 0]), 'without nodes or edges'),
        (dict(node_off=[1, 3]), 'node_off'), (dict(node_off=[0.0, 3.0]), 'node_off'), (dict(node_off=[0, 3, 6]), 'per graph'),
        (dict(edge_ids=[[0, 1], [1, 3]]), 'edge id outside'), (dict(edge_ids=[[0, -1], [1, 2]]), 'edge id outside'),
        (dict(edge_ids=[[0, 1], [2, 2]]), 'to itself'), (dict(edge_ids=[[0, 1]]), 'edge_ids must'),
        (dict(edge_ids=[[0.0, 1.0], [1.0, 2.0]]), 'edge_ids must'),
        (dict(edge_T=nan4), 'edge_T must be finite'), (dict(edge_T=np.eye(4)), 'edge_T must be'),
        (dict(edge_info=inf6), 'edge_info must be finite'), (dict(edge_info=np.zeros((2, 36))), 'edge_info must be'),
        (dict(pose_init=nanp), 'pose_init must be finite'), (dict(pose_init=nanp[:2]), 'pose_init must be'),
        (dict(edge_uncertain=[True]), 'edge_uncertain'),
        (dict(params=[(0.0, 0)]), 'mu must be positive'), (dict(params=[(-1.0, 0)]), 'mu must be positive'),
        (dict(params=[(float('nan'), 0)]), 'mu must be positive'), (dict(params=[(1.0, 3)]), 'reference node'),
        (dict(params=[(1.0, -1)]), 'reference node'), (dict(params=[(1.0, 0, -1)]), 'max_iter'),
        (dict(params=[(1.0, 0, 10, -1.0)]), 'rel_tol'), (dict(params=[(1.0, 0), (1.0, 0)]), 'per graph'),
    ]
    for change, match in cases:
        with pytest.raises(ValueError, match=match):
            ops.pose_graph_optimize(**dict(_tiny(), **change))
    with pytest.raises(ValueError, match='at most 128'):
        ops.pose_graph_optimize(**big)
    ops.check_pose_graph_args(**dict(big, node_off=[0, 128], pose_init=big['pose_init'][:128]))     # the cap itself passes
    # the method: the checks of score_pairs on the bank and the pairs, and its own, before the library is asked for anything
    off = [0, 4, 9, 12]
    bank = FragmentBank.from_tensors(torch.zeros(12, 4, dtype=torch.int32), torch.zeros(12, 3), torch.zeros(12, 16), off)
    dgr = DeepGlobalRegistration.__new__(DeepGlobalRegistration)
    dgr.device, dgr.voxel_size = torch.device('cuda'), 0.05
    pairs, T = [[0, 1], [1, 2]], np.tile(np.eye(4), (2, 1, 1))
    with pytest.raises(ValueError, match='the bank is on'):
        dgr.optimize_scene(bank, pairs, T)
    dgr.device = torch.device('cpu')
    scores = {'information': np.tile(np.eye(6), (2, 1, 1))}
    for kw, match in ((dict(pairs=[[0, 3]], T=T[:1]), 'pair id outside'), (dict(T=np.eye(4)), 'T must'),
                      (dict(radius=-1.0), 'radius'), (dict(reference_node=3), 'reference node'),
                      (dict(pairs=[[0, 1], [2, 2]]), 'to itself'), (dict(uncertain=[True]), 'uncertain flag'),
                      (dict(pose_init=np.eye(4)), 'pose_init'), (dict(edge_prune_threshold=2.0), 'edge_prune_threshold'),
                      (dict(scores={'information': np.zeros((2, 6, 6))}), 'no pair has a correspondence'),
                      (dict(scores={'information': np.zeros((1, 6, 6))}), 'information')):
        args = dict(dict(pairs=pairs, T=T, scores=scores), **kw)
        with pytest.raises(ValueError, match=match):
            dgr.optimize_scene(bank, args.pop('pairs'), args.pop('T'), **args)


def test_spanning_tree_pruning_connectivity_and_default_mu():
    rng = np.random.default_rng(0)
    P = np.stack([R.random_pose(rng) for _ in range(5)])
    P[0] = np.eye(4)
    rel = lambda s, t: pg.rigid_inverse(P[t]) @ P[s]
    # node 4 hangs on a certain edge only; (0, 2) is a heavier but WRONG uncertain edge: the tree must prefer certain ones
    edges = [(0, 1), (1, 2), (0, 2), (3, 2), (2, 3), (4, 3)]
    X = np.stack([rel(0, 1), rel(1, 2), R.random_pose(rng), rel(3, 2), R.random_pose(rng), rel(4, 3)])
    w = np.array([10.0, 10.0, 99.0, 30.0, 20.0, 5.0])
    unc = np.array([False, False, True, False, False, False])
    poses, reached = pg.spanning_tree_poses(5, edges, X, w, 0, unc)
    assert reached.all()
    np.testing.assert_allclose(poses, P, atol=1e-12)
    # without the preference the heaviest edge wins and the wrong X enters the tree
    wrong, _ = pg.spanning_tree_poses(5, edges, X, w, 0)
    assert np.abs(wrong[2] - P[2]).max() > 1e-3
    # among parallel edges the heavier (3, 2) is taken, not the wrong (2, 3)
    np.testing.assert_allclose(poses[3], P[3], atol=1e-12)
    # another reference node: the same relative poses, the reference at the identity
    q, _ = pg.spanning_tree_poses(5, edges, X, w, 3, unc)
    np.testing.assert_array_equal(q[3], np.eye(4))
    np.testing.assert_allclose(pg.rigid_inverse(q[0]) @ q[4], pg.rigid_inverse(P[0]) @ P[4], atol=1e-12)
    # a node nothing reaches is reported and keeps the identity
    poses, reached = pg.spanning_tree_poses(6, edges, X, w, 0, unc)
    assert reached.tolist() == [True] * 5 + [False]
    np.testing.assert_array_equal(poses[5], np.eye(4))
    with pytest.raises(ValueError, match='reference node'):
        pg.spanning_tree_poses(5, edges, X, w, 5)
    with pytest.raises(ValueError, match='edge id outside'):
        pg.spanning_tree_poses(3, edges, X, w, 0)
    # pruning: certain edges stay whatever their l; the threshold itself is kept
    kept = pg.prune_edges([0.0, 0.249, 0.25, 0.9, np.nan], [False, True, True, True, True])
    assert kept.tolist() == [True, False, True, True, False]
    assert pg.prune_edges([0.3, 0.3], [True, True], threshold=0.5).tolist() == [False, False]
    # connectivity through the kept edges
    e = [(0, 1), (1, 2), (3, 4), (2, 3)]
    assert pg.reachable_nodes(5, e).all()
    assert pg.reachable_nodes(5, e, [True, True, True, False]).tolist() == [True, True, True, False, False]
    assert pg.reachable_nodes(5, e, [True, True, True, False], reference_node=4).tolist() == [False, False, False, True, True]
    # mu = preference * d^2 * mean Lambda[3,3]; an edge at RMSE d has chi2 = mu and l = 1/4
    info = np.zeros((3, 6, 6))
    info[:, 3, 3] = (1000.0, 2000.0, 3000.0)
    assert pg.default_mu(info, 0.1) == pytest.approx(0.01 * 2000.0, rel=1e-15)
    assert pg.default_mu(info, 0.1, 2.0) == pytest.approx(0.02 * 2000.0, rel=1e-15)
    mu = pg.default_mu(info[1:2], 0.1)
    assert pg.line_process([mu], [True], mu)[0] == 0.25 and pg.line_process([mu], [False], mu)[0] == 1.0
    for bad in (dict(radius=0.0), dict(radius=float('nan')), dict(radius=0.1, preference_loop_closure=0.0)):
        with pytest.raises(ValueError):
            pg.default_mu(info, **bad)
    with pytest.raises(ValueError, match='no edges'):
        pg.default_mu(np.zeros((0, 6, 6)), 0.1)


def test_chi2_is_the_information_rmse_and_the_objective_is_its_robust_sum():
    from deepglobalregistration_amd.eval.metrics import information_rmse, rotation_vector
    g = R.make_graph(11, 7, 5)
    rng = np.random.default_rng(1)
    P = R.retract(rng.normal(scale=0.05, size=(7, 6)), g['P_init'])
    chi2 = pg.edge_chi2(P, g['edges'], g['X'], g['info'])
    for e, (s, t) in enumerate(g['edges']):
        rmse = information_rmse(np.linalg.inv(P[t]) @ P[s], g['X'][e], g['info'][e])
        assert chi2[e] == pytest.approx(g['info'][e, 3, 3] * rmse ** 2, rel=1e-11)
    unc, mu = g['uncertain'], g['mu']
    want = chi2[~unc].sum() + (mu * chi2[unc] / (mu + chi2[unc])).sum()
    assert pg.robust_objective(P, g['edges'], g['X'], g['info'], unc, mu) == pytest.approx(want, rel=1e-14)
    # F* is the minimum over l of the line-process objective, attained at line_process()
    l = pg.line_process(chi2, unc, mu)
    full = lambda l: chi2[~unc].sum() + (l[unc] * chi2[unc] + mu * (np.sqrt(l[unc]) - 1) ** 2).sum()
    assert full(l) == pytest.approx(want, rel=1e-13)
    for _ in range(5):
        assert full(np.clip(l + rng.normal(scale=0.05, size=len(l)), 0, 1)) >= want * (1 - 1e-14)
    # the stacked rotation vector is eval.metrics.rotation_vector, near 0 and near pi too
    axis = np.array([0.6, -0.48, 0.64])
    Rs = np.stack([R.so3_exp(axis * a) for a in (0.0, 1e-9, 1e-7, 1e-3, 1.0, 3.0, np.pi - 1e-7, np.pi - 1e-10, np.pi)])
    got = pg.rotation_vectors(Rs)
    for k in range(len(Rs)):
        np.testing.assert_allclose(got[k], rotation_vector(Rs[k]), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='mu must be positive'):
        pg.robust_objective(P, g['edges'], g['X'], g['info'], unc, 0.0)


def test_analytic_jacobians_match_central_differences():
    g = R.make_graph(5, 6, 3)
    rng = np.random.default_rng(2)
    P = R.retract(rng.normal(scale=0.3, size=(6, 6)), g['P_init'])      # away from the minimum: rotations up to ~1 rad
    X = g['X'].copy()
    # one edge whose E is a rotation near pi
    s, t = g['edges'][0]
    flip = np.eye(4)
    flip[:3, :3] = R.so3_exp(np.array([0.0, 0.0, np.pi - 1e-3]))
    X[0] = pg.rigid_inverse(flip) @ pg.rigid_inverse(P[t]) @ P[s]
    xi, J = R.edge_jacobians(P, g['edges'], X)
    assert abs(np.linalg.norm(xi[0, :3]) - (np.pi - 1e-3)) < 1e-9
    h, worst = 1e-6, 0.0
    for e, (s, t) in enumerate(g['edges']):
        for node, sign in ((s, 1.0), (t, -1.0)):
            for k in range(6):
                d = np.zeros((6, 6))
                d[node, k] = h
                xp = pg.edge_residuals(R.retract(d, P), g['edges'][e:e + 1], X[e:e + 1])[1][0]
                xm = pg.edge_residuals(R.retract(-d, P), g['edges'][e:e + 1], X[e:e + 1])[1][0]
                worst = max(worst, np.abs((xp - xm) / (2 * h) - sign * J[e][:, k]).max() / max(1.0, np.abs(J[e]).max()))
    # central differences at h = 1e-6: truncation h^2 |xi'''| ~ 1e-12, rounding eps |xi| / h ~ 1e-9
    assert worst < 1e-7, worst


@pytest.mark.parametrize('seed,n,k', [(0, 3, 0), (1, 8, 4), (2, 12, 10)])
def test_reference_solver_reaches_the_minimum_scipy_finds(seed, n, k):
    """The yardstick itself: the numpy LM and scipy's trust-region least squares on F*, from the same start, reach the same
    minimum -- F* to 1e-11 relative, poses to 1e-6 (measured: 4e-16 .. 1e-13 and 1e-10 .. 8e-9)."""
    g = R.make_graph(seed, n, k)
    a, b = R.lm_solve(*R.solve_args(g)), R.scipy_solve(*R.solve_args(g))
    assert a['converged'] and 3 <= a['iterations'] <= 40
    rel = abs(a['objective_final'] - b['objective_final']) / b['objective_final']
    dp = np.abs(a['poses'] - b['poses']).max()
    print(f'n={n}: F* {a["objective_initial"]:.6g} -> {a["objective_final"]:.15g} (scipy {b["objective_final"]:.15g}, rel {rel:.2e}), '
          f'pose diff {dp:.2e}, {a["iterations"]} steps')
    assert rel < 1e-11 and dp < 1e-6
    assert a['objective_final'] < a['objective_initial']
    np.testing.assert_array_equal(a['poses'][0], g['P_init'][0])
    l = a['line_process']
    assert (l[g['outlier']] < 1e-3).all() and (l[~g['outlier'] & g['uncertain']] > 0.45).all() and (l[~g['uncertain']] == 1).all()
    assert a['objective_final'] == pytest.approx(pg.robust_objective(a['poses'], g['edges'], X=g['X'], info=g['info'],
                                                                      uncertain=g['uncertain'], mu=g['mu']), rel=1e-14)


def test_scene_mode_writes_the_optimised_trajectory(tmp_path):
    """`eval.optimize_scenes` with a stand-in method: the trajectory holds the reachable fragments' poses, the second
    stats row judges inv(P_j) P_i, and a record with an unreachable fragment counts as a failure."""
    from deepglobalregistration_amd.eval import optimize_scenes, read_trajectory
    rng = np.random.default_rng(3)
    P = np.stack([R.random_pose(rng) for _ in range(4)])
    P[0] = np.eye(4)
    recs = [(0, 1), (1, 2), (0, 2), (2, 7)]                     # fragment ids of the files: 0, 1, 2, 7
    slot = {0: 0, 1: 1, 2: 2, 7: 3}
    T_true = {(i, j): pg.rigid_inverse(P[slot[j]]) @ P[slot[i]] for i, j in recs}

    class Dataset:
        scenes = ['room']
        def __len__(self): return len(recs)
        def records(self, s): return [(i, j, np.linalg.inv(T_true[i, j])) for i, j in recs]      # gt.log: pose = inv(T_gt)
        def fragment(self, s, f): return np.full((5, 3), float(f))

    class Method:
        use_icp = False
        def extract_fragments(self, clouds):
            assert [c[0, 0] for c in clouds] == [0.0, 1.0, 2.0, 7.0]
            return 'bank'
        def register_pairs(self, bank, pairs, batch_pairs, safeguard, icp):
            assert bank == 'bank' and pairs == [(0, 1), (1, 2), (0, 2), (2, 3)] and safeguard and not icp
            T = np.stack([T_true[r] for r in recs])
            T[2] = R.random_pose(rng)                            # a wrong pairwise estimate the graph repairs
            return T, np.zeros(4, np.int32), np.zeros((4, 4), np.float32)
        def optimize_scene(self, bank, pairs, T):
            return {'poses': P, 'reachable': np.array([True, True, True, False]), 'kept': np.array([True, True, False, False]),
                    'objective_initial': 2.0, 'objective_final': 1.0, 'iterations': 3}
    lines = []
    stats, rows = optimize_scenes(Method(), Dataset(), str(tmp_path / 'out'), out=lines.append)
    traj = read_trajectory(str(tmp_path / 'out' / 'room.log'))
    assert [m for m, _ in traj] == [[0, 0, 4], [1, 1, 4], [2, 2, 4]]
    for (m, pose) in traj:
        np.testing.assert_array_equal(pose, P[slot[m[0]]])
    assert stats.shape == (2, 4, 5)
    assert stats[0, :, 0].tolist() == [1, 1, 0, 1]               # pairwise: the wrong estimate fails
    assert stats[1, :, 0].tolist() == [1, 1, 1, 0]               # pose graph: repaired; the unreachable fragment fails
    assert np.isinf(stats[1, 3, 1]) and rows == [('room', 4, 3, 4, 2, 2.0, 1.0, 3)]
    assert any('pose graph' in ln for ln in lines)


# ----------------------------------------------------------------------------------------------------------------------
# the k-step comparison (posegraph_ref.steps_check): its yardstick, its tolerances and what it can see
_ALL = {**R.suite_graphs(), **R.step_graphs()}
_STEP_REF = {name: {} for name in _ALL}                    # name -> {k: lm_solve(max_iter=k)}, shared by the tests below
_SMALL = [name for name, g in _ALL.items() if g['n'] <= 20]


def _lm(**kw):
    return lambda g, k: R.lm_solve(*R.solve_args(g), max_iter=k, **kw)


def test_step_graphs_are_what_they_are_for():
    """The reject / re-damp loop really runs on the far starts, by the reference's own counter; the singular and
    rank-deficient graphs are solved, finite; the counters are consistent."""
    full = {name: R.lm_solve(*R.solve_args(g)) for name, g in R.step_graphs().items()}
    for name, r in full.items():
        print(f'{name}: {r["iterations"]} steps, {r["factorisations"]} factorisations, {r["rejections"]} rejected, '
              f'converged {r["converged"]}, F* {r["objective_initial"]:.6g} -> {r["objective_final"]:.6g}')
        assert r['converged'] and 1 <= r['iterations'] < 100 and np.isfinite(r['poses']).all()
        assert r['factorisations'] == r['iterations'] + r['rejections']
    assert full['far_n9']['rejections'] >= 4 and full['far_n13']['rejections'] >= 10
    assert full['rank1_info']['rejections'] >= 4
    g = R.step_graphs()['reference_last']
    assert g['reference_node'] == g['n'] - 1
    # max_iter = 0: nothing moves, nothing is factored
    g = _ALL['n5']
    r0 = R.lm_solve(*R.solve_args(g), max_iter=0)
    assert r0['iterations'] == 0 and not r0['converged'] and r0['factorisations'] == 0
    np.testing.assert_array_equal(r0['poses'], g['P_init'])
    with pytest.raises(ValueError):
        R.lm_solve(*R.solve_args(g), factor='lu')
    with pytest.raises(ValueError):
        R.lm_solve(*R.solve_args(g), mutant='none')


def test_k_step_noise_of_two_factorisations_and_the_gpu_tolerances():
    """The same k steps through two float64 factorisations of the same matrix (LAPACK's Cholesky; eigh + qr): their
    largest pose-entry difference per class is the noise the GPU test's STEP_TOL is ten times of (with the floor of 64
    ulp where the measured maximum is an ulp or two).  `steps_check` accepts the second factorisation on every graph at
    those tolerances, and the constants recorded in tests/test_gpu_pose_graph.py still bound what is measured here."""
    import test_gpu_pose_graph as G
    noise, entry = {c: 0.0 for c in G.STEP_TOL}, {c: 0.0 for c in G.STEP_TOL}
    for name, g in _ALL.items():
        c = R.step_class(name, g)
        rows = R.steps_check(_lm(factor='eigh_qr'), g, tol=G.STEP_TOL[c], reference=_STEP_REF[name])
        worst = max(dp for _, _, _, dp in rows)
        print(f'{name} [{c}]: |P_eigh_qr - P_cholesky| after k = {R.STEP_KS} steps: ' + ' '.join(f'{dp:.2e}' for _, _, _, dp in rows))
        noise[c] = max(noise[c], worst)
        entry[c] = max(entry[c], max(float(np.abs(ref['poses']).max()) for _, _, ref, _ in rows))
    undecided = {(name, k) for name in _ALL for k, ref in _STEP_REF[name].items()
                 if ref['decrease_ratio'] is not None and R.UNDECIDED[0] < ref['decrease_ratio'] < R.UNDECIDED[1]}
    assert undecided == {('n3_triangle', 5)}, undecided       # the one stopping decision `steps_check` leaves to rounding
    for c in G.STEP_TOL:
        print(f'class {c}: measured noise {noise[c]:.3e} (recorded {G.STEP_NOISE[c]:.3e}), largest pose entry {entry[c]:.3f}, '
              f'floor {G.STEP_FLOOR:.3e}, tolerance {G.STEP_TOL[c]:.3e}')
        assert G.STEP_TOL[c] == 10 * max(G.STEP_NOISE[c], G.STEP_FLOOR)
        assert 10 * noise[c] <= G.STEP_TOL[c]
        if G.STEP_NOISE[c] < G.STEP_FLOOR:      # the floor decides: it was taken in the binade of the class's largest entry
            assert 2.0 <= entry[c] < 4.0 and G.STEP_FLOOR == R.ulp64(entry[c])


def _old_criteria(g, ref, got, pose_tol):
    """The end-state criteria of test_gpu_pose_graph.test_reaches_the_reference_minimum, applied to a solver's result."""
    F = pg.robust_objective(got['poses'], g['edges'], g['X'], g['info'], g['uncertain'], g['mu'])
    line, out, unc = got['line_process'], g['outlier'], g['uncertain']
    return bool(F <= ref['objective_final'] * (1 + 1e-9) + 1e-12 and F <= ref['objective_initial']
                and (line[out] < 0.25).all() and (line[~out & unc] >= 0.25).all() and (line[~unc] == 1.0).all()
                and np.abs(got['poses'] - ref['poses']).max() <= pose_tol and got['converged'] and 1 <= got['iterations'] <= 100)


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_steps_check_rejects_what_the_end_state_criteria_let_through(mutant):
    """A solver with one deliberate error descends to the same minimum by another road: the end-state criteria pass it
    (printed: on which graphs), `steps_check` does not -- on every graph with an uncertain edge; the graphs without one
    cannot see 'weight_not_squared' (l = 1), and a single free node has no off-diagonal block to halve."""
    import test_gpu_pose_graph as G
    old, blind = [], []
    for name in _SMALL:
        g = _ALL[name]
        full_ref = R.lm_solve(*R.solve_args(g))
        full = R.lm_solve(*R.solve_args(g), mutant=mutant)
        if _old_criteria(g, full_ref, full, G.POSE_TOL):
            old.append(f'{name} ({full["iterations"]} steps, ref {full_ref["iterations"]})')
        try:
            R.steps_check(_lm(mutant=mutant), g, tol=G.STEP_TOL[R.step_class(name, g)], reference=_STEP_REF[name])
        except AssertionError as e:
            one = R.lm_solve(*R.solve_args(g), max_iter=1, mutant=mutant)
            print(f'{mutant} / {name}: rejected ({e}); pose difference after one step '
                  f'{np.abs(one["poses"] - _STEP_REF[name][1]["poses"]).max():.2e}')
            continue
        blind.append(name)
        assert not g['uncertain'].any(), f'steps_check accepted the mutant {mutant} on {name}'
    print(f'{mutant}: the end-state criteria pass it on {len(old)} of {len(_SMALL)} graphs: {old}')
    print(f'{mutant}: steps_check cannot see it on {blind}')


_PI_AXES = ((0.6, -0.48, 0.64), (0.6, -0.64, 0.48), (-0.8, 0.36, 0.48), (-0.6, -0.64, -0.48))
_PI_GAPS = (1e-3, 2e-6, 1.5e-6, 5e-7, 1e-8, 0.0)


@pytest.mark.parametrize('axis', _PI_AXES)
def test_rotation_vector_next_to_pi_for_any_axis(axis):
    """exp(log R) = R to 1e-10 for angle = pi - d on both sides of the switch to the symmetric part (sin(angle) = 1e-6;
    the antisymmetric branch just above it is at 2.6e-11 already), whatever the sign of the axis' largest entry: the
    symmetric part knows the axis up to its sign only.  At d = 0 both signs are logarithms."""
    from deepglobalregistration_amd.eval.metrics import rotation_vector
    a = np.array(axis) / np.linalg.norm(axis)
    for d in _PI_GAPS:
        Rm = R.so3_exp(a * (np.pi - d))
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = Rm, (0.3, -0.2, 0.5)
        E, xi = pg.edge_residuals(np.tile(np.eye(4), (2, 1, 1)), [[0, 1]], pg.rigid_inverse(X)[None])
        for what, w in (('metrics.rotation_vector', rotation_vector(Rm)), ('pose_graph.rotation_vectors', pg.rotation_vectors(Rm[None])[0]),
                        ('pose_graph.edge_residuals', xi[0, :3])):
            err = np.abs(R.so3_exp(w) - Rm).max()
            print(f'axis {axis} d={d:g} {what}: |exp(log R) - R| = {err:.2e}')
            assert err <= 1e-10, (what, axis, d, err)
            assert abs(np.linalg.norm(w) - (np.pi - d)) <= 1e-9
        np.testing.assert_allclose(xi[0, 3:], X[:3, 3], rtol=0, atol=1e-15)
