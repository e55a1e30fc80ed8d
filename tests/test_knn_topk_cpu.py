"""CPU: argument validation of the k-NN entry points happens before any device work; the knn_topk.npz goldens
reproduce from the reference's own core/knn.py on CPU torch (skipped where the reference is absent)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

BAD_K = [0, -1, 33, 100, 2.5, 2.0, True, '3', None]


def _no_device(*_a, **_k):
    raise AssertionError('device work started before the argument check')


def test_knn_argument_validation_before_device_work(monkeypatch):
    from deepglobalregistration_amd import _lib, ops
    from deepglobalregistration_amd.core import knn as cknn
    monkeypatch.setattr(_lib, 'load', _no_device)
    F0, F1 = torch.zeros(4, 32), torch.zeros(5, 32)
    lens = [(2, 3), (2, 2)]
    for k in BAD_K:
        for nn_max_n in (250, -1):
            with pytest.raises(ValueError, match='knn'):
                cknn.find_knn_gpu(F0, F1, nn_max_n=nn_max_n, knn=k)
            with pytest.raises(ValueError, match='knn'):
                cknn.find_knn_gpu_batch(F0, F1, lens, nn_max_n=nn_max_n, knn=k)
            with pytest.raises(ValueError, match='knn'):
                cknn.find_knn_batch(F0, F1, lens, nn_max_n=nn_max_n, knn=k)
        with pytest.raises(ValueError, match='knn'):
            ops.knn(F0, F1, k)
        with pytest.raises(ValueError, match='knn'):
            ops.knn_batch(F0, F1, [0, 2, 4], [0, 3, 5], k)


def test_knn_k_accepts_integers():
    from deepglobalregistration_amd import ops
    assert ops.KNN_MAX_K == 32
    for k in (1, 2, 32, np.int64(7), np.int32(32)):
        assert ops.check_knn_k(k) == int(k)


def test_knn_max_k_matches_header():
    from conftest import ROOT
    from deepglobalregistration_amd import ops
    text = open(os.path.join(ROOT, 'include', 'dgr_hip.h')).read()
    assert f'#define DGR_KNN_MAX_K {ops.KNN_MAX_K}\n' in text


def test_knn_topk_goldens_reproduce_from_reference():
    spec = importlib.util.spec_from_file_location('make_golden_knn_topk',
                                                  os.path.join(GOLDEN, 'make_golden_knn_topk.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.isfile(os.path.join(gen.REF, 'core', 'knn.py')):
        pytest.skip('the reference is not on this machine')
    pytest.importorskip('scipy')   # imported by the reference's core/knn.py
    out = gen.compute()
    g = np.load(os.path.join(GOLDEN, 'knn_topk.npz'))
    assert sorted(out) == sorted(g.files)
    for key in g.files:
        assert out[key].dtype == g[key].dtype and np.array_equal(out[key], g[key]), key
