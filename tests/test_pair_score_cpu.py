"""CPU-side checks of the pair scoring (csrc/pairscore.hip, core/pair_score.py): the C entry point exists, links from C
and refuses bad arguments before any device work; the Python wrappers refuse them before any device state exists; the
information matrix is the sum of G^T G it restates, predicts the squared residual of a small pose change to first order,
and survives the trajectory format; the conventions of an empty correspondence set."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _sums_of(q, d2=None):
    """The eleven sums of a correspondence set with the target points q [n,3] (float64, any summation order)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    s = np.zeros(11)
    s[0] = len(q)
    s[1] = 0.0 if d2 is None else float(np.sum(d2))
    s[2:5] = q.sum(0)
    s[5:] = [(q[:, a] * q[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return s


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def _se3_exp(omega, v):
    """exp of the twist (omega, v): R = exp([omega]x), t = V v (Rodrigues and its integral)."""
    th = float(np.linalg.norm(omega))
    K = _hat(omega)
    a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    E[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    return E


def _build_if_missing():
    from deepglobalregistration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_library_exports_the_entry_point():
    from deepglobalregistration_amd import _lib
    _build_if_missing()
    lib = _lib.load()
    assert 'dgr_score_pairs' in _lib.SIGNATURES
    assert hasattr(lib, 'dgr_score_pairs')


def test_entry_point_links_from_c_and_checks_arguments(tmp_path):
    """A C99 program links dgr_score_pairs and gets DGR_EINVAL for every bad argument the header lists -- reported before
    any device work, so the program needs no GPU (the context is a dummy non-NULL pointer)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    _build_if_missing()
    lib_dir = os.path.join(ROOT, 'deepglobalregistration_amd', 'lib')
    src = tmp_path / 'score_abi.c'
    src.write_text(r'''
#include <stdio.h>
#include <math.h>
#include "dgr_hip.h"
int main(void) {
  /* a context is only dereferenced behind the argument checks: any non-NULL pointer will do here */
  int dummy = 0; dgr_ctx *ctx = (dgr_ctx *)&dummy;
  float *xyz = (float *)&dummy;   /* a device pointer in real use: never dereferenced on the host */
  int64_t off[3] = {0, 4, 9}, off_neg[3] = {-1, 4, 9}, off_empty[3] = {0, 4, 4}, off_desc[3] = {0, 4, 2};
  int32_t ids[4] = {0, 1, 1, 1}, ids_hi[4] = {0, 1, 2, 0}, ids_neg[4] = {0, -1, 1, 0};
  double T[32] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1,  1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1}, Tnan[32], Tinf[32], Tlast[32];
  double out[2 * DGR_SCORE_WIDTH];
  int bad = 0, i;
  for (i = 0; i < 32; ++i) Tnan[i] = Tinf[i] = Tlast[i] = T[i];
  Tnan[16 + 3] = NAN; Tinf[5] = INFINITY; Tlast[12] = NAN;
  if (DGR_SCORE_WIDTH != 11) bad += 1;
  bad += dgr_score_pairs(0, xyz, off, 2, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, 0, off, 2, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, 0, 2, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, 0, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, 0, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, T, 0.1, 0, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 0, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, -3, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, T, 0.0, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, T, -0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, T, NAN, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, T, INFINITY, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, Tnan, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids, 2, Tinf, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off_neg, 2, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off_empty, 2, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off_desc, 2, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 0, ids, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids_hi, 2, T, 0.1, out, 0) != DGR_EINVAL;
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids_neg, 2, T, 0.1, out, 0) != DGR_EINVAL;
  /* the last row of a pose is ignored: a NaN there is no argument error (this call WOULD reach the device, so it is
     made with a pair id outside the bank: the only error left is that id) */
  bad += dgr_score_pairs(ctx, xyz, off, 2, ids_hi, 2, Tlast, 0.1, out, 0) != DGR_EINVAL;
  printf("%d %s\n", bad, dgr_last_error());
  return bad;
}
''')
    exe = tmp_path / 'score_abi'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    str(src), '-o', str(exe), '-L', lib_dir, '-ldgr_hip', f'-Wl,-rpath,{lib_dir}',
                    '-Wl,-rpath,/opt/rocm/lib', '-lm'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'fragment id 2 outside' in out.stdout     # the last call got past the pose check


def test_wrappers_reject_bad_arguments_before_any_device_state(monkeypatch):
    from deepglobalregistration_amd import _lib, ops
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    from deepglobalregistration_amd.util.pointcloud import compute_overlap_ratio
    import torch

    def no_device(*a, **k):
        raise AssertionError('device state touched before the argument check')
    monkeypatch.setattr(_lib, 'load', no_device)
    monkeypatch.setattr(ops, 'get_ctx', no_device)
    monkeypatch.setattr(ops, '_xyz_dev', no_device)
    monkeypatch.setattr(ops, 'voxelize', no_device)
    x = np.zeros((9, 3), np.float32)
    off, ids, T = [0, 4, 9], [[0, 1], [1, 0]], np.tile(np.eye(4), (2, 1, 1))
    for radius in (0.0, -0.1, float('nan'), float('inf'), '0.1', None, True):
        with pytest.raises(ValueError, match='radius'):
            ops.score_pairs(x, off, ids, T, radius)
    with pytest.raises(ValueError, match='radius'):
        compute_overlap_ratio(x, x, np.eye(4), 0.0)
    for bad_T in (np.eye(4), np.zeros((3, 4, 4)), np.zeros((2, 16)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match='T must'):
            ops.score_pairs(x, off, ids, bad_T, 0.1)
    for where in ((0, 0, 3), (1, 2, 2)):
        Tn = T.copy()
        Tn[where] = np.nan if where[0] else np.inf
        with pytest.raises(ValueError, match='finite'):
            ops.score_pairs(x, off, ids, Tn, 0.1)
    Tl = T.copy()
    Tl[1, 3, 0] = np.nan                         # the last row is ignored: the check passes and the call goes on
    assert ops.check_score_args(9, off, ids, Tl, 0.1)[2].shape == (2, 16)
    for bad_ids in ([[0, 2]], [[-1, 0]], [[0, 1], [1, 5]]):
        with pytest.raises(ValueError, match='pair id outside'):
            ops.score_pairs(x, off, bad_ids, np.tile(np.eye(4), (len(bad_ids), 1, 1)), 0.1)
    for empty in ([], np.zeros((0, 2), np.int64)):
        with pytest.raises(ValueError, match='empty'):
            ops.score_pairs(x, off, empty, np.zeros((0, 4, 4)), 0.1)
    for bad_ids in ([0, 1], [[0, 1, 1]], [[0.0, 1.0]]):
        with pytest.raises(ValueError, match='pair_ids must'):
            ops.score_pairs(x, off, bad_ids, np.eye(4)[None], 0.1)
    for bad_off in ([0, 4, 8], [0, 4, 4, 9], [0, 5, 4, 9], [-1, 4, 9], [9], [0.0, 9.0]):
        with pytest.raises(ValueError, match='bank_off'):
            ops.score_pairs(x, bad_off, [[0, 0]], np.eye(4)[None], 0.1)
    with pytest.raises(ValueError, match=r'\[N,3\]'):
        ops.score_pairs(np.zeros((9, 2), np.float32), off, ids, T, 0.1)
    # the method: same checks on the bank and the pairs as register_pairs, before the library is asked for anything
    bank = FragmentBank.from_tensors(torch.zeros(9, 4, dtype=torch.int32), torch.zeros(9, 3), torch.zeros(9, 16), off)
    dgr = DeepGlobalRegistration.__new__(DeepGlobalRegistration)    # (no networks are needed to refuse an argument)
    dgr.device, dgr.voxel_size = torch.device('cuda'), 0.05
    with pytest.raises(ValueError, match='the bank is on'):
        dgr.score_pairs(bank, ids, T)
    dgr.device = torch.device('cpu')             # (a device the bank is on: the remaining checks are reached)
    with pytest.raises(ValueError, match='pair id outside'):
        dgr.score_pairs(bank, [[0, 2]], np.eye(4)[None])
    with pytest.raises(ValueError, match='empty'):
        dgr.score_pairs(bank, [], np.zeros((0, 4, 4)))
    with pytest.raises(ValueError, match='T must'):
        dgr.score_pairs(bank, ids, np.eye(4))
    with pytest.raises(ValueError, match='radius'):
        dgr.score_pairs(bank, ids, T, radius=-1.0)
    with pytest.raises(ValueError, match='inverted'):
        dgr.score_pairs(bank, ids, np.zeros((2, 4, 4)))


def test_information_matrix_is_the_sum_of_GtG():
    from deepglobalregistration_amd.core.pair_score import information_from_sums
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (500, 3)) * [4.0, 3.5, 2.6] + [0.5, -1.0, 2.0]
    x, y, z = q.T
    o, l = np.zeros(500), np.ones(500)
    G = np.stack((np.stack((o, z, -y, l, o, o), 1), np.stack((-z, o, x, o, l, o), 1), np.stack((y, -x, o, o, o, l), 1)), 1)
    want = np.einsum('nij,nik->jk', G, G)
    got = information_from_sums(_sums_of(q))
    assert got.shape == (1, 6, 6)
    err = np.abs(got[0] - want).max() / np.abs(want).max()
    print(f'closed form against the row sum: relative error {err:.2e}')
    assert err < 1e-12
    np.testing.assert_array_equal(got[0][3:, 3:], 500 * np.eye(3))
    np.testing.assert_array_equal(got[0], got[0].T)
    two = information_from_sums(np.stack((_sums_of(q), _sums_of(q[:7]))))
    np.testing.assert_array_equal(two[0], got[0])
    np.testing.assert_array_equal(two[1][3:, 3:], 7 * np.eye(3))
    with pytest.raises(ValueError, match=r'\[n,11\]'):
        information_from_sums(np.zeros((2, 10)))


@pytest.mark.parametrize('w_norm', [1e-2, 1e-3, 1e-4])
def test_information_matrix_predicts_the_residual_to_first_order(w_norm):
    """xi^T Lambda xi against sum |E q - q|^2 for E = exp(xi), |omega| = w_norm and |v| between 0.1 and 3 times that, points
    uniform in a 4 x 3.5 x 2.6 m box: the relative difference is below 5 |omega| (the neglected terms are second order in
    omega: about |omega| / 2 relative; the bound leaves a tenfold margin).  `information_rmse` reads the twist back from the
    two poses and must match the direct RMSE under the same bound."""
    from deepglobalregistration_amd.core.pair_score import information_from_sums
    from deepglobalregistration_amd.eval.metrics import information_rmse
    rng = np.random.default_rng(1)
    worst = worst_rmse = 0.0
    for draw in range(200):
        q = rng.uniform(0, 1, (300, 3)) * [4.0, 3.5, 2.6]
        omega = rng.normal(size=3)
        omega *= w_norm / np.linalg.norm(omega)
        v = rng.normal(size=3)
        v *= w_norm * rng.uniform(0.1, 3.0) / np.linalg.norm(v)
        xi = np.concatenate((omega, v))
        E = _se3_exp(omega, v)
        info = information_from_sums(_sums_of(q))[0]
        direct = float((((q @ E[:3, :3].T + E[:3, 3]) - q) ** 2).sum())
        worst = max(worst, abs(float(xi @ info @ xi) - direct) / direct)
        T = _se3_exp(rng.normal(size=3), rng.normal(size=3))
        rmse = information_rmse(E @ T, T, info)
        want = np.sqrt(direct / len(q))
        worst_rmse = max(worst_rmse, abs(rmse - want) / want)
    print(f'|omega| = {w_norm:g}: worst relative difference {worst / w_norm:.3f} |omega| (quadratic form), '
          f'{worst_rmse / w_norm:.3f} |omega| (information_rmse)')
    assert worst < 5 * w_norm
    assert worst_rmse < 5 * w_norm


def test_information_rmse_conventions():
    from deepglobalregistration_amd.eval.metrics import information_rmse, rotation_vector
    T = _se3_exp(np.array([0.3, -0.2, 0.5]), np.array([1.0, 2.0, -0.5]))
    assert information_rmse(T, T, np.zeros((6, 6))) == float('inf')
    info = np.diag([3.0, 4.0, 5.0, 10.0, 10.0, 10.0])
    assert information_rmse(T, T, info) < 1e-15
    # a pure translation: exactly its length, whatever the points were
    E = np.eye(4)
    E[:3, 3] = [0.03, -0.04, 0.12]
    assert abs(information_rmse(E @ T, T, info) - 0.13) < 1e-12
    with pytest.raises(ValueError, match=r'\[6,6\]'):
        information_rmse(T, T, np.zeros((4, 4)))
    for w in ([0.3, -0.2, 0.5], [1e-9, 0, 0], [0, 0, 0], [0, np.pi - 1e-9, 0], [2.0, -2.0, 1.0]):
        w = np.asarray(w, np.float64)
        np.testing.assert_allclose(rotation_vector(_se3_exp(w, np.zeros(3))[:3, :3] if w.any() else np.eye(3)), w, atol=1e-7)


def test_information_records_survive_the_trajectory_format(tmp_path):
    from deepglobalregistration_amd.core.pair_score import information_from_sums
    from deepglobalregistration_amd.eval.formats import read_trajectory, write_trajectory
    rng = np.random.default_rng(2)
    infos = information_from_sums(np.stack([_sums_of(rng.normal(size=(n, 3)) * 3.3) for n in (1, 40, 1234)]))
    records = [([0, 1, 60], infos[0]), ([0, 7, 60], infos[1]), ([58, 59, 60], infos[2])]
    path = tmp_path / 'scene.info'
    write_trajectory(str(path), records)
    back = read_trajectory(str(path), dim=6)
    assert [m for m, _ in back] == [m for m, _ in records]
    for (_, a), (_, b) in zip(back, records):
        np.testing.assert_array_equal(a, b)


def test_scores_from_sums_conventions():
    from deepglobalregistration_amd.core.pair_score import scores_from_sums
    s = np.zeros((3, 11))
    s[1, :2] = [8, 0.02]
    s[2, :2] = [10, 0.0]
    out = scores_from_sums(s, [5, 16, 10])
    assert out['n_corr'].tolist() == [0, 8, 10] and out['n_corr'].dtype == np.int64
    assert out['fitness'].tolist() == [0.0, 0.5, 1.0]
    assert out['inlier_rmse'].tolist() == [0.0, 0.05, 0.0]
    assert out['information'].shape == (3, 6, 6) and not out['information'][0].any()
    assert np.isfinite(out['fitness']).all() and np.isfinite(out['inlier_rmse']).all()
    one = scores_from_sums(s[1], [16])
    assert one['fitness'].tolist() == [0.5]
    with pytest.raises(ValueError, match='one source row count'):
        scores_from_sums(s, [5, 16])
