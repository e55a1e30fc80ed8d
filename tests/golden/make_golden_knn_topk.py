"""Golden vectors of the k-NN search (knn > 1) from the REFERENCE's own `core/knn.py`.

Run where the reference is importable (DGR_REFERENCE, as for make_golden.py):

    python tests/golden/make_golden_knn_topk.py

`find_knn_gpu` / `find_knn_gpu_batch` of the reference run unchanged on CPU torch (one thread: summation order
independent of the host) and their outputs land in knn_topk.npz next to this script.  tests/test_knn_topk_cpu.py
recomputes them from the reference where it exists; tests/test_gpu_knn_topk.py compares the HIP search with them.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get('DGR_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'knn_topk.npz')


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def inputs():
    """The seeded inputs of every case: name -> dict of arrays (the F0 / F1 of a case and its batch sizes)."""
    rng = np.random.default_rng(2024)
    cases = {}
    cases['c32'] = dict(F0=_unit(rng.standard_normal((200, 32))), F1=_unit(rng.standard_normal((450, 32))))
    cases['c16'] = dict(F0=_unit(rng.standard_normal((120, 16))), F1=_unit(rng.standard_normal((260, 16))))
    cases['c64'] = dict(F0=_unit(rng.standard_normal((80, 64))), F1=_unit(rng.standard_normal((200, 64))))
    # exact ties: F1 rows 40.. repeat rows 0..39, F0 holds copies of some of them (distance 0, twice)
    F1 = _unit(rng.standard_normal((80, 32)))
    F1[40:] = F1[:40]
    F0 = np.concatenate([F1[5:25], _unit(rng.standard_normal((30, 32)))])
    cases['ties'] = dict(F0=F0, F1=F1)
    # k > N1: five references; and the issue's one-dimensional example, F1 = {0, 1, 1, 3} x 1, query 0.9 x 1
    cases['short'] = dict(F0=_unit(rng.standard_normal((20, 32))), F1=_unit(rng.standard_normal((5, 32))))
    cases['example'] = dict(F0=np.full((1, 32), 0.9, np.float32),
                            F1=(np.array([0, 1, 1, 3], np.float32)[:, None] * np.ones((1, 32), np.float32)))
    # a collated batch of three pairs (base_loader collation: rows back to back)
    lens = np.array([[60, 150], [40, 7], [80, 160]], np.int64)
    cases['batch'] = dict(F0=_unit(rng.standard_normal((int(lens[:, 0].sum()), 32))),
                          F1=_unit(rng.standard_normal((int(lens[:, 1].sum()), 32))), lens=lens)
    return cases


# (case, knn) searched in both branches of find_knn_gpu
SINGLE = [('c32', 2), ('c32', 3), ('c32', 8), ('c16', 3), ('c64', 8), ('ties', 2), ('ties', 3), ('short', 8),
          ('example', 6)]
BATCH_K = [3, 8]


def compute(ref=REF):
    if ref not in sys.path:
        sys.path.insert(0, ref)
    from core.knn import find_knn_gpu, find_knn_gpu_batch
    torch.set_num_threads(1)
    out = {}
    cases = inputs()
    for name, arrs in cases.items():
        for key, a in arrs.items():
            out[f'{name}_{key}'] = a
    for name, k in SINGLE:
        F0, F1 = torch.from_numpy(cases[name]['F0']), torch.from_numpy(cases[name]['F1'])
        ic, dc = find_knn_gpu(F0, F1, nn_max_n=250, knn=k, return_distance=True)
        iu, du = find_knn_gpu(F0, F1, nn_max_n=-1, knn=k, return_distance=True)
        out.update({f'{name}_k{k}_idx_chunked': ic.numpy(), f'{name}_k{k}_dist_chunked': dc.numpy(),
                    f'{name}_k{k}_idx_unchunked': iu.numpy(), f'{name}_k{k}_dist_unchunked': du.numpy()})
    b = cases['batch']
    F0, F1, lens = torch.from_numpy(b['F0']), torch.from_numpy(b['F1']), b['lens'].tolist()
    for k in BATCH_K:
        per_i, per_d = find_knn_gpu_batch(F0, F1, lens, nn_max_n=250, knn=k, return_distance=True)
        cat_i, cat_d = find_knn_gpu_batch(F0, F1, lens, nn_max_n=250, knn=k, return_distance=True,
                                          concat_results=True)
        for p, (i, d) in enumerate(zip(per_i, per_d)):
            out[f'batch_k{k}_pair{p}_idx'] = i.numpy()
            out[f'batch_k{k}_pair{p}_dist'] = d.numpy()
        out[f'batch_k{k}_cat_idx'] = cat_i.numpy()
        out[f'batch_k{k}_cat_dist'] = cat_d.numpy()
    return out


def main():
    out = compute()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
