"""GPU: the batched k-NN searches per pair -- every route, descriptor table and list boundary -- on the cases of
tests/knn_cases.py (proved on the CPU by tests/test_knn_cases_cpu.py), with the library's route trace
(ops.knn_trace / ops.knn_trace_rows) telling which kernels searched each pair.

One child process per mode (tests/aux/knn_routes_dump.py: plain, then DGR_KNN_BRUTE=1 -- not started unless the first
exited 0, each under its own timeout) dumps every result of tests a - d and the trace rows; the tests below share the
two dumps and one float64 reference.
  a  70 pairs in tables of 32 + 32 + 6, every table starting (table 1 also ending) on the brute-force route, fallback /
     dup33 / list65 (top-k: list257) / aligned pairs on call positions 1, 31, 33, 69 and -- in the reversed order --
     32, 63, 64: every pair equals its own single-pair call, the prefiltered run equals the brute-force run byte for
     byte, float64 agrees (EQUAL indices on the rows certified tie-free, which is every row of the big, dup*, list* and
     aligned pairs; ascending rows inside the duplicate clusters; distances within 1e-6), and a pair's bytes do not depend
     on its place, table or neighbours (reversed, shuffled).
  b  the routes, from the trace.  Exact for 1-NN: dup32 -> 32 candidates and no list, dup33 -> 33 and a list of 40,
     list64 -> 64 without redo, list65 -> 65 with (list64w / list65w: the same beside 330 duplicates, where a list
     nobody redoes also returns wrong rows).  Top-k: list256 -> 256 without redo, list257 -> 257 with, asserted
     exactly for every k: beside the cluster U is a duplicate's distance whatever the device samples (1025 duplicates fill
     every slot class many times over), and the pairs' other queries stay hundreds of candidates below their slot counts.
  c  40 pairs each of width 16 and 64 (brute force throughout), 1-NN and k = 8.
  d  the bound: one aligned pair of 1500 queries; column 0 is the float64 neighbour although the decoy ranks 0.22 tau
     ahead of it in the approximate distances.  With KNN_TAU_C / 8 this test fails (1-NN: every query).
  e  the search inside dgr_register_batch (34 pairs, two tables) and dgr_register_pairs (36 directed pairs of a
     9-fragment bank) against ops.knn1_batch and ops.knn1 on the features the call used."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import knn_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
PAIR, TABLE, ROUTE, FALLBACK, LIST_LEN, REDO, CAND_MAX, CAND_ZERO = range(8)


@pytest.fixture(scope='module')
def cases():
    return dict(batch1=kc.batch(False), batchk=kc.batch(True), bound=kc.bound_pair(),
                width16=kc.width_batch(16), width64=kc.width_batch(64))


@pytest.fixture(scope='module')
def dumps(cases, tmp_path_factory):
    d = tmp_path_factory.mktemp('knn_routes')
    with open(d / 'cases.pkl', 'wb') as f:
        pickle.dump(cases, f)
    out, secs = {}, {}
    for mode in ('plain', 'brute'):
        env = {k: v for k, v in os.environ.items() if k != 'DGR_KNN_BRUTE'}
        if mode == 'brute':
            env['DGR_KNN_BRUTE'] = '1'
        t0 = time.time()
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'aux', 'knn_routes_dump.py'),
                            str(d / f'{mode}.npz'), str(d / 'cases.pkl')], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
        secs[mode] = time.time() - t0
        assert p.returncode == 0, f'{mode}: the dump ended with {p.returncode}\n{(p.stdout + p.stderr)[-3000:]}'
        with np.load(d / f'{mode}.npz') as z:
            out[mode] = {k: z[k] for k in z.files}
    print('knn routes dumps: ' + ', '.join(f'{k} {v:.1f} s' for k, v in secs.items()) + f", {len(out['plain'])} keys")
    return out


@pytest.fixture(scope='module')
def ref(cases):
    """float64 top-33 of every pair of a and c, computed once."""
    out = {}
    for name in ('batch1', 'batchk', 'width16', 'width64'):
        for p in cases[name]:
            if id(p) not in out:
                out[id(p)] = kc.f64_topk(p.F0, p.F1)
    return out


def _pairs(cases, k):
    return cases['batch1'] if k == 1 else cases['batchk']


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _offsets(pairs, order):
    _, _, off0, off1 = kc.concat(pairs, order)
    return off0, off1


# ---- a ---------------------------------------------------------------------------------------------------------------
def test_a_every_pair_equals_its_single_pair_call(dumps):
    for mode in ('plain', 'brute'):
        z = dumps[mode]
        for k in kc.KS:
            for sq in (0, 1):
                for what in ('idx', 'dist'):
                    assert _same(z[f'a_k{k}_base_sq{sq}_{what}'], z[f'a_k{k}_single_sq{sq}_{what}']), (mode, k, sq, what)


def test_a_prefiltered_run_equals_brute_force_run(dumps):
    keys = sorted(k for k in dumps['plain'] if not k.endswith('_trace'))
    assert keys == sorted(k for k in dumps['brute'] if not k.endswith('_trace')) and len(keys) >= 2 * 2 * 4 * 4
    for key in keys:
        assert _same(dumps['plain'][key], dumps['brute'][key]), key


def _check_f64(p, top, k, idx, dist, squared, certify=True):
    """One pair against float64: idx [n0, k] pair-local, dist [n0, k].  certify: equal indices on the tie-free rows (else
    the suite's tie rule on every row)."""
    ridx, rD = top
    kk = min(k, p.n1)
    assert np.all(idx[:, kk:] == 0) and np.all(np.isinf(dist[:, kk:]))          # padding: index 0 of the pair, inf
    assert idx[:, :kk].min() >= 0 and idx[:, :kk].max() < p.n1
    idx, dist, ridx, rD = idx[:, :kk], dist[:, :kk], ridx[:, :kk], rD[:, :kk]
    certified = kc.tie_free(*top, k, p.cluster) if certify else np.zeros(p.n0, bool)
    if p.kind in ('big', 'dup32', 'dup33', 'list64', 'list65', 'list64w', 'list65w', 'list256', 'list257', 'aligned'):
        assert certified.all()
    np.testing.assert_array_equal(idx[certified], ridx[certified])
    D = kc.d2_f64_of(p.F0, p.F1, idx)
    rest = ~certified
    if rest.any():                                                              # elsewhere: the suite's tie rule
        assert np.abs(D[rest] - rD[rest]).max() <= kc.TIE_TOL
    if p.cluster is not None:                                                   # inside a cluster: ascending rows
        m = min(kk, p.cluster[1] - p.cluster[0])
        np.testing.assert_array_equal(idx[p.near, :m], np.tile(np.arange(p.cluster[0], p.cluster[0] + m), (len(p.near), 1)))
    np.testing.assert_allclose(dist, D if squared else np.sqrt(D + 1e-7), atol=1e-6)
    assert np.all(np.diff(dist, axis=1) >= 0)


def test_a_against_float64(dumps, cases, ref):
    z = dumps['plain']
    for k in kc.KS:
        pairs = _pairs(cases, k)
        off0, off1 = _offsets(pairs, None)
        for sq in (0, 1):
            idx, dist = z[f'a_k{k}_base_sq{sq}_idx'].astype(np.int64), z[f'a_k{k}_base_sq{sq}_dist']
            assert idx.shape == dist.shape == (off0[-1], k)
            for j, p in enumerate(pairs):
                rows = slice(off0[j], off0[j + 1])
                _check_f64(p, ref[id(p)], k, idx[rows] - off1[j], dist[rows], sq)


def test_a_a_pair_does_not_depend_on_its_place(dumps, cases):
    orders = kc.orders()
    for mode in ('plain', 'brute'):
        z = dumps[mode]
        for k in kc.KS:
            pairs = _pairs(cases, k)
            b0, b1 = _offsets(pairs, orders['base'])
            for name in ('reversed', 'shuffled'):
                o0, o1 = _offsets(pairs, orders[name])
                for sq in (0, 1):
                    bi, bd = z[f'a_k{k}_base_sq{sq}_idx'], z[f'a_k{k}_base_sq{sq}_dist']
                    oi, od = z[f'a_k{k}_{name}_sq{sq}_idx'], z[f'a_k{k}_{name}_sq{sq}_dist']
                    for j, p in enumerate(orders[name]):
                        there, here = slice(o0[j], o0[j + 1]), slice(b0[p], b0[p + 1])
                        assert np.array_equal(oi[there] - o1[j], bi[here] - b1[p]), (mode, k, name, sq, j, int(p))
                        assert _same(od[there], bd[here]), (mode, k, name, sq, j, int(p))


# ---- b ---------------------------------------------------------------------------------------------------------------
def _check_row(p, k, row, where):
    """The trace row of pair p searched with k on the prefilter-enabled run."""
    if not p.prefiltered:
        assert row[ROUTE] == 0 and not row[FALLBACK:].any(), (where, row)
        return
    assert row[ROUTE] == 1, (where, row)
    if p.kind == 'fallback':
        assert row[FALLBACK] == 1 and (k == 1 or row[REDO] == 1), (where, row)   # 1-NN: the fallback flag IS the redo
        return
    assert row[FALLBACK] == 0, (where, row)
    assert row[CAND_ZERO] == 0, (where, row)           # pass 2 re-finds at least the sampled minimum of every query
    assert row[REDO] == (p.kind in (('list65', 'list65w') if k == 1 else ('list257',))), (where, row)
    if p.kind == 'aligned':
        assert row[LIST_LEN] == 0, (where, row)
    if k == 1:
        want = {'dup32': (32, 0), 'dup33': (33, 40), 'list64': (33, 64), 'list65': (33, 65), 'list64w': (330, 64),
                'list65w': (330, 65)}.get(p.kind)
        if want:
            assert (row[CAND_MAX], row[LIST_LEN]) == want, (where, row)
    elif p.kind in ('list256', 'list257'):
        assert row[LIST_LEN] == len(p.near) == int(p.kind[4:]), (where, row)
        assert row[CAND_MAX] == p.cluster[1] - p.cluster[0], (where, row)


def test_b_routes_from_the_trace(dumps, cases):
    orders = kc.orders()
    for k in kc.KS:
        pairs = _pairs(cases, k)
        assert {'list65' if k == 1 else 'list257', 'dup32', 'dup33', 'fallback', 'aligned'} <= {p.kind for p in pairs}
        for name, order in list(orders.items()) + [('single', orders['base'])]:
            tr = dumps['plain'][f'a_k{k}_{name}_trace']
            assert tr.shape == (70, 8) and tr.dtype == np.int32
            assert np.array_equal(tr[:, PAIR], np.arange(70))
            assert np.array_equal(tr[:, TABLE], np.arange(70) // kc.KNN_MAXP if name != 'single' else np.zeros(70))
            for j, p in enumerate(order):
                _check_row(pairs[int(p)], k, tr[j], (k, name, j, pairs[int(p)].kind))
            br = dumps['brute'][f'a_k{k}_{name}_trace']                         # the other run: brute force throughout
            assert br.shape == (70, 8) and np.array_equal(br[:, :2], tr[:, :2]) and not br[:, ROUTE:].any()
    assert dumps['plain']['off_trace'].shape == (0, 8)                          # switched off: nothing recorded


# ---- c ---------------------------------------------------------------------------------------------------------------
def test_c_other_widths(dumps, cases, ref):
    for C in (16, 64):
        pairs = cases[f'width{C}']
        off0, off1 = _offsets(pairs, None)
        for mode in ('plain', 'brute'):
            z = dumps[mode]
            for k in (1, 8):
                tr = z[f'c{C}_k{k}_base_trace']
                assert np.array_equal(tr[:, PAIR], np.arange(40)) and np.array_equal(tr[:, TABLE], np.arange(40) // 32)
                assert not tr[:, ROUTE:].any() and not z[f'c{C}_k{k}_single_trace'][:, TABLE:].any()
                for sq in (0, 1):
                    idx, dist = z[f'c{C}_k{k}_base_sq{sq}_idx'], z[f'c{C}_k{k}_base_sq{sq}_dist']
                    assert _same(idx, z[f'c{C}_k{k}_single_sq{sq}_idx']) and _same(dist, z[f'c{C}_k{k}_single_sq{sq}_dist'])
                    if mode == 'brute':
                        continue
                    for j, p in enumerate(pairs):
                        rows = slice(off0[j], off0[j + 1])
                        _check_f64(p, ref[id(p)], k, idx[rows].astype(np.int64) - off1[j], dist[rows], sq, certify=False)


# ---- d ---------------------------------------------------------------------------------------------------------------
def test_d_the_bound_keeps_the_true_neighbour(dumps, cases):
    p = cases['bound']
    assert p.n0 == 1500 and p.meta['inversion'].min() > 0.2      # the decoy is AHEAD by a fifth of tau, emulated
    for k in (1, 2, 8):
        tr = dumps['plain'][f'd_k{k}_single_trace']
        assert tr.shape == (1, 8) and tr[0].tolist()[:6] == [0, 0, 1, 0, 0, 0] and tr[0, CAND_ZERO] == 0, tr
        for sq in (0, 1):
            idx, dist = dumps['plain'][f'd_k{k}_single_sq{sq}_idx'], dumps['plain'][f'd_k{k}_single_sq{sq}_dist']
            wrong = np.nonzero(idx[:, 0] != p.meta['nn'])[0]
            assert len(wrong) == 0, (k, sq, len(wrong), wrong[:8], idx[wrong[:8], 0], p.meta['nn'][wrong[:8]])
            D = kc.d2_f64_of(p.F0, p.F1, idx.astype(np.int64))
            np.testing.assert_allclose(dist, D if sq else np.sqrt(D + 1e-7), atol=1e-6)
            assert _same(idx, dumps['brute'][f'd_k{k}_single_sq{sq}_idx'])
            assert _same(dist, dumps['brute'][f'd_k{k}_single_sq{sq}_dist'])


# ---- e ---------------------------------------------------------------------------------------------------------------
def _check_fused(n1_of, off0, off1):
    """After a fused call with the trace on: its rows, and its matches against the k-NN entries on the features it used."""
    from deepglobalregistration_amd import ops
    tr = ops.knn_trace_rows('cuda')
    n = len(off0) - 1
    assert tr.shape == (n, 8) and np.array_equal(tr[:, PAIR], np.arange(n)) and np.array_equal(tr[:, TABLE], np.arange(n) // 32)
    assert np.array_equal(tr[:, ROUTE], [int(n1_of(p) >= kc.KNN_MIN_REFS) for p in range(n)])
    assert not tr[:, FALLBACK].any() and not tr[tr[:, ROUTE] == 1, CAND_ZERO].any()
    F0, F1 = (ops.batch_output('cuda', key).reshape(-1, 32) for key in ('F0', 'F1'))
    idx1 = ops.batch_output('cuda', 'idx1')
    assert len(F0) == off0[-1] == len(idx1) and len(F1) == off1[-1]
    assert torch.equal(idx1, ops.knn1_batch(F0, F1, off0, off1))
    for p in range(n):
        alone = ops.knn1(F0[off0[p]:off0[p + 1]], F1[off1[p]:off1[p + 1]])
        assert torch.equal(idx1[off0[p]:off0[p + 1]] - int(off1[p]), alone), p
    return tr


def test_e_search_inside_the_fused_calls():
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    voxel = 0.05
    ck = synth.synth_checkpoint(seed=0, voxel_size=voxel, feat_conv1_kernel_size=7)
    dgr = DeepGlobalRegistration({'weights': ck, 'clip_weight_thresh': 0.05}, torch.device('cuda'))
    rng = np.random.default_rng(5)
    clouds = [synth.synth_pair(s, n_raw=2500)[:2] for s in range(34)]
    clouds[7] = (rng.uniform(0, 0.4, (60, 3)), rng.uniform(0, 0.4, (45, 3)))          # tens of voxels
    clouds[33] = (clouds[33][0], np.array([[0.01, 0.02, 0.03]]))                       # a one-voxel fragment
    x0, c0, x1, c1, off0, off1 = [], [], [], [], [0], [0]
    for p, (a, b) in enumerate(clouds):
        xa, ca, _ = dgr.preprocess(a, batch_index=p)
        xb, cb, _ = dgr.preprocess(b, batch_index=p)
        x0.append(xa); c0.append(ca); x1.append(xb); c1.append(cb)
        off0.append(off0[-1] + len(xa)); off1.append(off1[-1] + len(xb))
    assert off1[34] - off1[33] == 1
    ops.knn_trace('cuda', True)
    try:
        dgr.register_voxelized(torch.cat(c0), torch.cat(x0), off0, torch.cat(c1), torch.cat(x1), off1)
        tr = _check_fused(lambda p: off1[p + 1] - off1[p], off0, off1)
        assert tr[:, ROUTE].sum() >= 30 and tr[7, ROUTE] == 0 and tr[33, ROUTE] == 0 and tr[33, TABLE] == 1
        # the same through register_pairs: a 9-fragment bank, 36 directed pairs in one call
        scene, _, _ = synth.synth_scene(3, 9, n_raw=2500)
        bank = dgr.extract_fragments(scene)
        ids = [(i, j) if (i + j) % 2 else (j, i) for i in range(9) for j in range(i + 1, 9)]
        assert len(ids) == 36
        dgr.register_pairs(bank, ids, batch_pairs=36)
        size = np.diff(np.asarray(bank.off))
        o0 = np.concatenate([[0], np.cumsum([size[i] for i, _ in ids])])
        o1 = np.concatenate([[0], np.cumsum([size[j] for _, j in ids])])
        tr = _check_fused(lambda p: size[ids[p][1]], o0, o1)
        assert tr[35, TABLE] == 1 and tr[:, ROUTE].all()
    finally:
        ops.knn_trace('cuda', False)
    assert ops.knn_trace_rows('cuda').shape == (0, 8)
