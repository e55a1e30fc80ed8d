"""CPU side of the o3d.hip edge tests: the preconditions of the shared cases (tests/o3d_cases.py), the references of
tests/o3d_ref.py against each other, and a NumPy model of the ICP's sum form which the bound must reject when the sums
are taken in absolute coordinates far from the origin and accept when they are taken relative to the centre of the target's box."""
import numpy as np
import pytest

import o3d_cases as oc
import o3d_ref as ref
from oracle import open3d_reg as o3


# ---- preconditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', oc.ORACLE_CASES)
def test_oracle_cases_are_decided(name):
    """At every evaluation of the oracle's run no match lies within relative 1e-6 of max_dist^2 and no nearest / second
    nearest pair within relative 1e-9 of each other; the instrumented run IS the oracle's."""
    c, tr = oc.icp_case(name), oc.oracle_trace(name)
    assert tr['margin'] > 1e-6 and tr['gap'] > 1e-9, (name, tr['margin'], tr['gap'])
    T, f, r, it = o3.icp_point_to_point(c['src'], c['dst'], c['max_dist'], init=c['init'], **c['kw'])
    assert it == tr['iterations'] and f == tr['fitness'] and r == tr['rmse'] and np.array_equal(T, tr['T'])


@pytest.mark.parametrize('name', oc.EXACT_CASES + oc.RANK1_CASES)
def test_one_step_cases_are_decided(name):
    c = oc.icp_case(name)
    nn = oc.brute(name)
    fin = np.isfinite(nn.d2)
    assert nn.margin[fin].min() > 1e-6 and nn.gap[fin & (nn.d2 < 4 * c['max_dist'] ** 2)].min() > 1e-9
    assert (nn.idx >= 0).sum() >= 2


def test_sizes_and_layouts():
    assert [len(oc.icp_case(f'n0:{n}')['src']) for n in oc.SIZES_N0] == list(oc.SIZES_N0)
    assert ref.n_blocks(65537) == 257                                  # one more block partial than the solve has threads
    c = oc.icp_case('cell_doubling')
    cell, dims, doublings = oc.layout(c['dst'], c['max_dist'])
    assert doublings == 2 and cell == 0.4 and dims.tolist() == [100, 100, 100]
    assert np.prod(np.floor(39.9 / np.array([0.1, 0.2])) + 1) ** 3 > oc.CELL_CAP   # 400^3 and 200^3 are over the cap
    assert oc.oracle_trace('cell_doubling')['fitness'] > 0.9
    c = oc.icp_case('flat_axis')
    assert np.ptp(c['dst'][:, 2]) == 0 and oc.layout(c['dst'], c['max_dist'])[1][2] == 1
    assert oc.layout(oc.icp_case('n1:1')['dst'], 0.1)[1].tolist() == [1, 1, 1]
    assert oc.oracle_trace('n1:1')['matches'][0] == 300


def test_negative_side_cases():
    c = oc.icp_case('negative_far')
    lo = c['dst'].astype(np.float64).min(0)
    assert (c['src'].max(0) < lo - 45).all() and oc.oracle_trace('negative_far')['fitness'] == 0
    c = oc.icp_case('negative_faces')
    d8 = c['dst'].astype(np.float64)
    lo, hi, P = d8.min(0), d8.max(0), oc.placed(c)
    assert (c['src'].max(0) < lo - 45).all()                           # the raw source: 50 units below the grid
    cell = np.floor((P - lo) / c['max_dist'])
    dims = oc.layout(c['dst'], c['max_dist'])[1]
    nn = ref.nearest_bruteforce(P, c['dst'], c['max_dist'])
    for ax in range(3):                                                # matched points one cell outside each face
        assert ((cell[:, ax] == -1) & (nn.idx >= 0)).sum() >= 5 and ((cell[:, ax] == dims[ax]) & (nn.idx >= 0)).sum() >= 5


def test_criteria_and_few_matches():
    for k, its in oc.CRITERIA_ITERATIONS.items():
        assert oc.oracle_trace(f'criteria:{k}')['iterations'] == its, k
    for k in (0, 1, 3):
        assert oc.oracle_trace(f'few_matches:{k}')['matches'][0] == k
    c = oc.icp_case('few_matches:2')
    nn = ref.nearest_bruteforce(oc.placed(c), c['dst'], c['max_dist'])
    assert (nn.idx >= 0).sum() == 2 and len(set(nn.idx[nn.idx >= 0])) == 2
    c = oc.icp_case('n1:2')
    nn = ref.nearest_bruteforce(oc.placed(c), c['dst'], c['max_dist'])
    assert (nn.idx >= 0).sum() > 250 and set(nn.idx[nn.idx >= 0]) == {0, 1}


def test_mirror_case_is_a_reflection():
    c = oc.icp_case('mirror')
    nn = ref.nearest_bruteforce(c['src'], c['dst'], c['max_dist'])
    assert (nn.idx >= 0).all()
    P, Q = c['src'].astype(np.float64), c['dst'].astype(np.float64)[nn.idx]
    assert np.array_equal(P[:, :2], Q[:, :2]) and np.array_equal(P[:, 2], -Q[:, 2])      # every point matches its own image
    sigma = np.array([[float(v) for v in row] for row in ref.exact_moments(P, Q)[2]])
    ex = ref.umeyama_exact(P, Q)
    assert np.linalg.det(sigma) < 0 and ex.sg == -1.0 and abs(np.linalg.det(ex.T[:3, :3]) - 1) < 1e-12
    T, f, _, it = o3.icp_point_to_point(c['src'], c['dst'], c['max_dist'], **c['kw'])
    assert it == 1 and f == 1.0 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12 and np.abs(T - ex.T).max() < 1e-12


def test_ties_are_exact():
    src, dst, rev, perm = oc.ties()
    nn = ref.nearest_bruteforce(src, dst, oc.MAX_DIST)
    assert (nn.gap == 0).all() and (nn.idx >= 0).all()
    e = dst.astype(np.float64)[None] - src.astype(np.float64)[:7, None]
    assert ((e * e).sum(-1) == nn.d2[:7, None]).sum(1).tolist() == [8] * 7
    assert sorted(map(tuple, rev)) == sorted(map(tuple, dst)) == sorted(map(tuple, perm))


# ---- the references against each other ---------------------------------------------------------------------------------
def _matched(name):
    c = oc.icp_case(name)
    P = oc.placed(c)
    nn = oc.brute(name)
    ok = nn.idx >= 0
    return c, P[ok], c['dst'].astype(np.float64)[nn.idx[ok]]


def test_umeyama_exact_against_the_oracle_near_the_origin():
    _, P, Q = _matched('one_step:0')
    ex = ref.umeyama_exact(P, Q)
    assert len(P) > 2000 and np.abs(ex.T - o3.umeyama(P, Q)).max() < 1e-13
    X, Y = oc.corr_problem(513)
    S = o3.ransac_samples(0, 0, 50, 513)
    for s in S:
        assert np.abs(ref.umeyama_exact(X[s], Y[s]).T - o3.umeyama(X[s], Y[s])).max() < 1e-12
    assert np.array_equal(ref.umeyama_exact(np.zeros((0, 3)), np.zeros((0, 3))).T, np.eye(4))


@pytest.mark.parametrize('offset', oc.OFFSETS)
def test_umeyama_exact_against_mpmath(offset):
    mp = pytest.importorskip('mpmath')
    _, P, Q = _matched(f'one_step:{offset}')
    P, Q = P[::5], Q[::5]
    with mp.workdps(60):
        Pm, Qm = mp.matrix(P.tolist()), mp.matrix(Q.tolist())
        n = len(P)
        one = mp.ones(1, n)
        mpm, mqm = one * Pm / n, one * Qm / n
        sig = (Qm - mp.ones(n, 1) * mqm).T * (Pm - mp.ones(n, 1) * mpm) / n
        U, s, V = mp.svd_r(sig)
        sg = -1 if mp.det(U) * mp.det(V) < 0 else 1
        R = U * mp.diag([1, 1, sg]) * V
        t = mqm.T - R * mpm.T
        Rm, tm = np.array(R.tolist(), dtype=np.float64), np.array([float(v) for v in t])
    ex = ref.umeyama_exact(P, Q)
    # the yardstick's own error in R: the SVD's backward error seen through the rotation's conditioning (s1 / gap) plus
    # the three roundings per entry of the product U diag(1, 1, sg) V^T -- 8 eps64 for the lot
    own = 8 * ref.EPS64 * (1 + ex.s[0] / ex.gap)
    assert np.abs(ex.T[:3, :3] - Rm).max() <= own
    assert np.abs(ex.T[:3, 3] - tm).max() <= own * np.abs(ex.mp).sum() + 2 * ref.EPS64 * np.abs(tm).max()
    assert np.allclose([float(v) for v in s], ex.s, rtol=1e-12)


def test_consensus_is_the_oracles_inline_statement():
    X, Y = oc.corr_problem(513)
    thr2 = np.float32(np.float32(0.1) * np.float32(0.1))
    S = o3.ransac_samples(3, 0, 40, 513)
    for s in S:
        T = o3.umeyama(X[s].astype(np.float64), Y[s].astype(np.float64))
        R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
        p0 = (R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1]) + R[0, 2] * X[:, 2] + t[0]
        p1 = (R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1]) + R[1, 2] * X[:, 2] + t[1]
        p2 = (R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1]) + R[2, 2] * X[:, 2] + t[2]
        e0, e1, e2 = p0 - Y[:, 0], p1 - Y[:, 1], p2 - Y[:, 2]
        d2 = (e0 * e0 + e1 * e1) + e2 * e2
        inl = d2 < thr2
        err = float(np.add.accumulate(d2[inl], dtype=np.float32)[-1]) if inl.any() else 0.0
        assert ref.consensus(T, X, Y, thr2) == (int(inl.sum()), err)
    assert ref.consensus(np.eye(4), X, X + np.float32(1), thr2) == (0, 0.0)


# ---- the bound against a model of the sum form -------------------------------------------------------------------------
def model_sum_form(P, Q, origin):
    """The device's arithmetic in NumPy f64: 17 sums of coordinates relative to `origin`, the covariance as
    Sqp / n - mq mp^T, LAPACK SVD, t moved back by t' + o - R o."""
    o = np.asarray(origin, np.float64)
    Pp, Qp = P - o, Q - o
    n = len(P)
    mp_, mq_ = Pp.sum(0) / n, Qp.sum(0) / n
    sig = (Qp.T @ Pp) / n - np.outer(mq_, mp_)
    U, _, Vt = np.linalg.svd(sig)
    sg = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1, 1, sg]) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (mq_ - R @ mp_) + (o - R @ o)
    return T


@pytest.mark.parametrize('offset', oc.OFFSETS)
def test_bound_separates_absolute_from_relative_sums(offset):
    c, P, Q = _matched(f'one_step:{offset}')
    corner = c['dst'].astype(np.float64).min(0)
    nb = ref.n_blocks(len(c['src']))
    d8 = c['dst'].astype(np.float64)
    ratio_rel = ref.check_T(model_sum_form(P, Q, 0.5 * (d8.min(0) + d8.max(0))), P, Q, nb, corner)[0]   # the kernel's origin
    ratio_abs, eR, bR, et, bt = ref.check_T(model_sum_form(P, Q, np.zeros(3)), P, Q, nb, corner)
    ratio_oracle = ref.check_T(o3.umeyama(P, Q), P, Q, nb, corner)[0]
    print(f'offset {offset}: relative sums {ratio_rel:.2e}, absolute sums {ratio_abs:.2e} (R {eR:.1e}/{bR:.1e}, t {et:.1e}/{bt:.1e}), '
          f'centred oracle {ratio_oracle:.2e} of the bound')
    assert ratio_rel <= 1 and ratio_oracle <= 1
    if offset == 1000:
        assert ratio_abs > 10                      # sums in absolute coordinates 1000 units out: visibly rejected
    if offset == 0:
        assert ratio_abs <= 1


# ---- RANSAC cases -----------------------------------------------------------------------------------------------------
def test_ransac_case_preconditions():
    for n in oc.TILE_N:
        for seed in oc.TILE_SEEDS:
            assert oc.distinct_samples(n, 2000, seed)[0].min() >= 3, (n, seed)
    nd, S = oc.distinct_samples(4, 3000, 0)
    tuples = {}
    for h, s in enumerate(map(tuple, S.tolist())):
        tuples.setdefault(s, []).append(h)
    assert len(tuples) == 256 and max(map(len, tuples.values())) >= 20 and (nd < 3).sum() > 1000
    first = np.array([v[0] for v in tuples.values()])
    later = np.array([v[-1] for v in tuples.values()])
    assert (later // 64 != first // 64).any() and (later // 256 != first // 256).any()     # repeats across waves and blocks
    for n in oc.REPEAT_N:
        assert oc.repeat_best_distinct(n, 3000, 0) >= 2
    X, Y, T, h, c, r = oc.ransac_non_finite()
    bad = ~(np.isfinite(X).all(1) & np.isfinite(Y).all(1))
    assert bad.sum() == 4 and c > 100 and np.isfinite(T).all()
    assert bad[o3.ransac_samples(0, 0, 2000, 600)].any(1).sum() > 10
