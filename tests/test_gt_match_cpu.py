"""CPU-side checks of the ground-truth matching and validation statistics: the three C entry points exist and are
callable from C, the Python wrappers reject bad arguments before any device state exists, the statistic arithmetic of
`validate_collated` reproduces the reference's formulas, and the committed goldens are what the reference computes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ('dgr_radius_pairs_batch', 'dgr_pairs_isin_batch', 'dgr_validation_counts')


def test_library_exports_the_three_entry_points():
    from deepglobalregistration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_entry_points_link_from_c_and_check_arguments(tmp_path):
    """A C99 program links the three entry points and gets DGR_EINVAL for NULL / bad arguments -- reported before any
    device work, so the program needs no GPU."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    lib_dir = os.path.join(ROOT, 'deepglobalregistration_amd', 'lib')
    if not os.path.exists(os.path.join(lib_dir, 'libdgr_hip.so')):
        import __graft_entry__ as g
        g.build()
    src = tmp_path / 'gt_abi.c'
    src.write_text(r'''
#include <stdio.h>
#include <math.h>
#include "dgr_hip.h"
int main(void) {
  /* a context is only dereferenced behind the argument checks: any non-NULL pointer will do here */
  int dummy = 0; dgr_ctx *ctx = (dgr_ctx *)&dummy;
  int64_t off[2] = {0, 4}, bad_off[2] = {0, -1}, total = -1, M[1] = {4}, counts[6];
  double T[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1}, Tnan[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
  float xyz[12] = {0}; int32_t cnt[4]; uint8_t lab[4] = {0}; float w[4] = {0};
  int bad = 0;
  Tnan[3] = NAN;
  bad += dgr_radius_pairs_batch(ctx, xyz, off, xyz, off, 1, T, 0.0, 0, cnt, 0, 0, &total, 0) != DGR_EINVAL;
  bad += dgr_radius_pairs_batch(ctx, xyz, off, xyz, off, 1, T, -1.0, 0, cnt, 0, 0, &total, 0) != DGR_EINVAL;
  bad += dgr_radius_pairs_batch(ctx, xyz, off, xyz, off, 1, T, 0.1, -1, cnt, 0, 0, &total, 0) != DGR_EINVAL;
  bad += dgr_radius_pairs_batch(ctx, xyz, bad_off, xyz, off, 1, T, 0.1, 0, cnt, 0, 0, &total, 0) != DGR_EINVAL;
  bad += dgr_radius_pairs_batch(ctx, xyz, off, xyz, off, 1, Tnan, 0.1, 0, cnt, 0, 0, &total, 0) != DGR_EINVAL;
  bad += dgr_radius_pairs_batch(0, xyz, off, xyz, off, 1, T, 0.1, 0, cnt, 0, 0, &total, 0) != DGR_EINVAL;
  bad += dgr_pairs_isin_batch(ctx, 0, bad_off, 0, off, 1, M, lab, 0) != DGR_EINVAL;
  bad += dgr_pairs_isin_batch(0, 0, off, 0, off, 1, M, lab, 0) != DGR_EINVAL;
  bad += dgr_validation_counts(ctx, lab, w, 0.5f, bad_off, 1, counts, 0) != DGR_EINVAL;
  bad += dgr_validation_counts(ctx, lab, w, 0.5f, off, 0, counts, 0) != DGR_EINVAL;
  printf("%d %s\n", bad, dgr_last_error());
  return bad;
}
''')
    exe = tmp_path / 'gt_abi'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    str(src), '-o', str(exe), '-L', lib_dir, '-ldgr_hip', f'-Wl,-rpath,{lib_dir}',
                    '-Wl,-rpath,/opt/rocm/lib', '-lm'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_wrappers_reject_bad_arguments_before_any_device_state(monkeypatch):
    from deepglobalregistration_amd import _lib, ops
    from deepglobalregistration_amd.util.pointcloud import get_matching_indices

    def no_device(*a, **k):
        raise AssertionError('device state touched before the argument check')
    monkeypatch.setattr(_lib, 'load', no_device)
    monkeypatch.setattr(ops, 'get_ctx', no_device)
    monkeypatch.setattr(ops, '_xyz_dev', no_device)
    x = np.zeros((5, 3), np.float32)
    T = np.eye(4)
    for radius in (0.0, -0.1, float('nan'), float('inf'), '0.1', None, True):
        with pytest.raises(ValueError, match='radius'):
            ops.radius_pairs(x, x, T, radius)
    with pytest.raises(ValueError, match='radius'):
        get_matching_indices(x, x, T, 0)
    for K in (0, -1, 1.5, True, '2'):
        with pytest.raises(ValueError, match='K must'):
            ops.radius_pairs(x, x, T, 0.1, K)
    for bad_T in (np.eye(3), np.zeros((2, 4, 4)), np.zeros(16)):
        with pytest.raises(ValueError, match='T must'):
            ops.radius_pairs(x, x, bad_T, 0.1)
    Tn = np.eye(4)
    Tn[0, 3] = np.inf
    with pytest.raises(ValueError, match='finite'):
        ops.radius_pairs(x, x, Tn, 0.1)
    for off0 in ([0, 3, 2, 5], [1, 5], [0, 4], [0]):
        with pytest.raises(ValueError, match='off0'):
            ops.radius_pairs_batch(x, off0, x, [0, 5] if len(off0) == 2 else [0, 1, 2, 5], np.tile(np.eye(4), (len(off0) - 1, 1, 1)), 0.1)
    with pytest.raises(ValueError, match='same number of pairs'):
        ops.radius_pairs_batch(x, [0, 5], x, [0, 2, 5], T[None], 0.1)
    with pytest.raises(ValueError, match=r'\[N,3\]'):
        ops.radius_pairs(np.zeros((5, 2)), x, T, 0.1)
    pairs = np.zeros((4, 2), np.int64)
    with pytest.raises(ValueError, match='pos_off'):
        ops.pairs_isin(pairs, [0, 3], pairs, [0, 4], [4])
    with pytest.raises(ValueError, match='same number of pairs'):
        ops.pairs_isin(pairs, [0, 4], pairs, [0, 4], [4, 4])
    with pytest.raises(ValueError, match=r'\[N,2\]'):
        ops.pairs_isin(np.zeros((4, 3), np.int64), [0, 4], pairs, [0, 4], [4])
    with pytest.raises(ValueError, match='off'):
        ops.validation_counts(np.zeros(4, np.uint8), np.zeros(4, np.float32), [0, 5])
    with pytest.raises(ValueError, match='one entry per'):
        ops.validation_counts(np.zeros(4, np.uint8), np.zeros(3, np.float32), [0, 4])
    with pytest.raises(ValueError, match='threshold'):
        ops.validation_counts(np.zeros(4, np.uint8), np.zeros(4, np.float32), [0, 4], threshold=float('nan'))


def test_find_correct_correspondence_keeps_the_reference_assertions():
    from deepglobalregistration_amd.core.correspondence import find_correct_correspondence
    p = [np.zeros((1, 2), np.int64)]
    with pytest.raises(AssertionError):
        find_correct_correspondence(p, p + p, hash_seed=3)
    with pytest.raises(AssertionError):
        find_correct_correspondence(p, p, len_batch=[[1, 1], [1, 1]])


def test_validation_statistics_are_the_trainer_formulas():
    """core/trainer.py:443-448 written out on hand-made counts (eps = np.finfo(float).eps, :34)."""
    from deepglobalregistration_amd.eval.metrics import VALID_EPS, batch_rte_rre, validation_statistics
    eps = np.finfo(float).eps
    assert VALID_EPS == eps
    #                  n  hits tp fp tn fn
    counts = np.array([[10, 4, 3, 2, 4, 1],
                       [6, 5, 5, 0, 1, 0],
                       [0, 0, 0, 0, 0, 0]], np.int64)
    tp, fp, tn, fn = 8, 2, 5, 1
    precision = tp / (tp + fp + eps)
    recall = tp / (tp + fn + eps)
    f1 = 2 * (precision * recall) / (precision + recall + eps)
    tpr = tp / (tp + fn + eps)
    tnr = tn / (tn + fp + eps)
    s = validation_statistics(counts)
    assert s == {'hit_ratio': 9 / 16, 'precision': precision, 'recall': recall, 'f1': f1, 'tpr': tpr, 'tnr': tnr,
                 'balanced_accuracy': (tpr + tnr) / 2}
    # nothing predicted, nothing positive: the eps keeps every ratio finite (0 / eps = 0), as in the reference
    z = validation_statistics(np.array([[5, 0, 0, 0, 5, 0]]))
    assert z['precision'] == 0 and z['recall'] == 0 and z['f1'] == 0 and z['tnr'] == 5 / (5 + eps) and z['hit_ratio'] == 0
    assert validation_statistics(np.zeros((1, 6), np.int64))['hit_ratio'] == 0
    # a perfect classifier reads 1 / (1 + eps / tp): "exactly 1" in float64 for any realistic count
    one = validation_statistics(np.array([[100, 100, 100, 0, 0, 0]]))
    assert one['precision'] == 1.0 and one['recall'] == 1.0 and one['hit_ratio'] == 1.0
    # RTE / RRE as _valid_epoch measures them: the reference clamps the cosine to +-0.999
    ang = np.radians(10.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    T_gt = np.tile(np.eye(4), (2, 1, 1))
    rte, rre = batch_rte_rre(np.stack((R, np.eye(3))), np.array([[0.3, 0.4, 0.0], [0, 0, 0]]), T_gt)
    np.testing.assert_allclose(rte, [0.5, 0.0], atol=1e-15)
    np.testing.assert_allclose(rre, [10.0, np.degrees(np.arccos(0.999))], rtol=1e-12)


def test_goldens_are_the_reference_output():
    """Where the reference is present: its find_correct_correspondence gives the committed labels, and the restated brute
    force gives the committed radius pairs."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_gt_match', os.path.join(GOLDEN, 'make_golden_gt_match.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    if not os.path.exists(os.path.join(mg.REF, 'core', 'correspondence.py')):
        pytest.skip('the reference is not on this machine')
    try:
        fresh = mg.compute()
    finally:
        for p in (mg.REF, os.path.join(GOLDEN, 'me_stub')):
            while p in sys.path:
                sys.path.remove(p)
    stored = np.load(os.path.join(GOLDEN, 'gt_match.npz'))
    assert sorted(stored.files) == sorted(fresh)
    for k in stored.files:
        np.testing.assert_array_equal(stored[k], fresh[k], err_msg=k)
    assert stored['label_collide'].sum() > 0 and 0 < stored['label_default'].mean() < 1
    assert os.path.getsize(os.path.join(GOLDEN, 'gt_match.npz')) < 64 * 1024
