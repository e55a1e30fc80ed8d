"""Helper of tests/test_gpu_knn_routes.py: every k-NN call of its tests a - d once, with the route trace on, into one
.npz (results as they come back plus the trace rows of every call).

    [DGR_KNN_BRUTE=1] python tests/aux/knn_routes_dump.py OUT.npz [CASES.pkl]

The brute-force switch is read once per process, hence one process per mode.  CASES.pkl: the cases of tests/knn_cases.py
as the test built them (dict: batch1, batchk, bound, width16, width64); without it they are built here.
Keys: <test>_k<k>_<order | single>_sq<0|1>_{idx,dist} and ..._trace (squared = 0 only; `single`: one row per pair, the
row of its own one-pair call with the pair's call position written into field 0)."""
import os
import pickle
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: knn_cases
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the package
import knn_cases as kc   # noqa: E402
from deepglobalregistration_amd import ops   # noqa: E402

DEV = 'cuda'
OUT = {}


def _search(F0, F1, off0, off1, k, squared):
    """One batched call (off0 given) or one single-pair call: (idx, dist) on the device, [n0, k]."""
    if off0 is None:
        idx, dist = (ops.knn1(F0, F1, squared=squared, return_distance=True) if k == 1 else
                     ops.knn(F0, F1, k, squared=squared, return_distance=True))
    else:
        idx, dist = (ops.knn1_batch(F0, F1, off0, off1, squared=squared, return_distance=True) if k == 1 else
                     ops.knn_batch(F0, F1, off0, off1, k, squared=squared, return_distance=True))
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32
    return idx.reshape(len(F0), k), dist.reshape(len(F0), k)


def _put(key, idx, dist):
    OUT[f'{key}_idx'] = idx.cpu().numpy().astype(np.int32)      # (rows of F1: far below 2^31)
    OUT[f'{key}_dist'] = dist.cpu().numpy()


def run_batch(tag, pairs, ks, orders):
    for name, order in orders.items():
        F0, F1, off0, off1 = kc.concat(pairs, order)
        T0, T1 = torch.from_numpy(F0).to(DEV), torch.from_numpy(F1).to(DEV)
        for k in ks:
            for sq in (0, 1):
                idx, dist = _search(T0, T1, off0, off1, k, bool(sq))
                if sq == 0:
                    OUT[f'{tag}_k{k}_{name}_trace'] = ops.knn_trace_rows(DEV)
                _put(f'{tag}_k{k}_{name}_sq{sq}', idx, dist)
        if name != 'base':
            continue
        for k in ks:                                            # every pair alone, written in the batch's numbering
            for sq in (0, 1):
                ii, dd, tr = [], [], []
                for p in range(len(pairs)):
                    i, d = _search(T0[off0[p]:off0[p + 1]], T1[off1[p]:off1[p + 1]], None, None, k, bool(sq))
                    ii.append(i + int(off1[p]))
                    dd.append(d)
                    if sq == 0:
                        rows = ops.knn_trace_rows(DEV)
                        assert rows.shape == (1, 8) and rows[0, 0] == 0 and rows[0, 1] == 0, rows
                        rows[0, 0] = p
                        tr.append(rows[0])
                _put(f'{tag}_k{k}_single_sq{sq}', torch.cat(ii), torch.cat(dd))
                if sq == 0:
                    OUT[f'{tag}_k{k}_single_trace'] = np.stack(tr)


def main(out_path, cases_path=None):
    if cases_path:
        with open(cases_path, 'rb') as f:
            cases = pickle.load(f)
    else:
        cases = dict(batch1=kc.batch(False), batchk=kc.batch(True), bound=kc.bound_pair(),
                     width16=kc.width_batch(16), width64=kc.width_batch(64))
    assert ops.knn_trace_rows(DEV).shape == (0, 8)             # nothing recorded before the switch
    ops.knn_trace(DEV, True)
    orders = kc.orders()
    run_batch('a', cases['batch1'], (1,), orders)
    run_batch('a', cases['batchk'], (2, 8, 32), orders)
    base = {'base': orders['base'][:40]}
    run_batch('c16', cases['width16'], (1, 8), base)
    run_batch('c64', cases['width64'], (1, 8), base)
    b = cases['bound']                                          # d: ONE pair, through the single-pair entries
    T0, T1 = torch.from_numpy(b.F0).to(DEV), torch.from_numpy(b.F1).to(DEV)
    for k in (1, 2, 8):
        for sq in (0, 1):
            idx, dist = _search(T0, T1, None, None, k, bool(sq))
            if sq == 0:
                OUT[f'd_k{k}_single_trace'] = ops.knn_trace_rows(DEV)
            _put(f'd_k{k}_single_sq{sq}', idx, dist)
    # the switch: off again, a call records nothing and the old rows are gone
    ops.knn_trace(DEV, False)
    p = cases['batch1'][1]
    ops.knn1(torch.from_numpy(p.F0).to(DEV), torch.from_numpy(p.F1).to(DEV))
    OUT['off_trace'] = ops.knn_trace_rows(DEV)
    np.savez(out_path, **OUT)


if __name__ == '__main__':
    main(*sys.argv[1:3])
