"""CPU-side checks of the k-NN route trace (dgr_ctx_set_knn_trace / dgr_debug_knn_trace): the library exports the two
entries with the declared signatures, and the `ops` wrappers refuse anything that is not a GPU device before any device
state exists (no context, no library call)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def test_trace_symbols_exist_and_are_declared():
    from deepglobalregistration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dgr_hip.h')).read()
    for name in ('dgr_ctx_set_knn_trace', 'dgr_debug_knn_trace'):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert re.search(r'\bint\s+%s\s*\(\s*dgr_ctx\s*\*ctx' % name, header), name
    assert _lib.SIGNATURES['dgr_ctx_set_knn_trace'] == (C.c_int, [_lib.vp, C.c_int])
    res, args = _lib.SIGNATURES['dgr_debug_knn_trace']
    assert res is C.c_int and args == [_lib.vp, _lib.c_i32p, C.c_int64, C.POINTER(C.c_int64)]
    # a NULL context is an argument error, not a crash
    assert lib.dgr_ctx_set_knn_trace(None, 1) == _lib.DGR_EINVAL
    n = C.c_int64(-1)
    assert lib.dgr_debug_knn_trace(None, None, 0, C.byref(n)) == _lib.DGR_EINVAL


@pytest.mark.parametrize('bad', [None, 0, 3, True, 1.5, 'cpu', 'not-a-device', object(), [0]])
def test_trace_wrappers_refuse_a_non_device(bad, monkeypatch):
    from deepglobalregistration_amd import _lib, ops

    def no_ctx(*a, **k):
        raise AssertionError('a context was asked for')
    monkeypatch.setattr(ops, 'get_ctx', no_ctx)
    monkeypatch.setattr(_lib, 'get_ctx', no_ctx)
    with pytest.raises(ValueError):
        ops.knn_trace(bad, True)
    with pytest.raises(ValueError):
        ops.knn_trace_rows(bad)
    assert getattr(_lib._tls, 'ctx', None) is None


def test_trace_wrappers_refuse_a_tensor():
    import torch
    from deepglobalregistration_amd import ops
    with pytest.raises(ValueError):
        ops.knn_trace(torch.zeros(2), True)
    with pytest.raises(ValueError):
        ops.knn_trace_rows(torch.zeros(2))
    assert len(ops.KNN_TRACE_FIELDS) == 8
