"""The ICP and the safeguard RANSAC of csrc/o3d.hip at their edges (tests/o3d_cases.py): against the KD-tree oracle where
the oracle's run is decided (tests/test_o3d_edges_cpu.py asserts that), against an exact Umeyama of the brute-force matches
within a bound computed from the inputs (tests/o3d_ref.py) where one step is probed, and by their properties where the
rotation is not unique.  Every case reports its worst ratio to its bound (DGR_PARITY_REPORT, o3d_edges_vs_exact.txt)."""
import numpy as np
import pytest
import torch

import o3d_cases as oc
import o3d_ref as ref
from oracle import open3d_reg as o3
from reg_checks import report

pytestmark = pytest.mark.gpu
FILE = 'o3d_edges_vs_exact.txt'


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()


def _icp(case, dst=None, **override):
    from deepglobalregistration_amd import ops
    kw = oc.ops_kw(case)
    kw.update(override)
    return ops.icp_point_to_point(_dev(case['src']), _dev(case['dst'] if dst is None else dst), case['max_dist'],
                                  init=case['init'], **kw)


def _ransac(X, Y, hyp, seed):
    from deepglobalregistration_amd import ops
    return ops.ransac_correspondence(_dev(X), _dev(Y), oc.RS_THR, hyp, seed=seed)


def _is_rotation(T):
    R = T[:3, :3]
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


# ---- ICP --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', oc.ORACLE_CASES)
def test_icp_matches_oracle(name):
    """Iteration count, fitness, rmse and T as tests/test_gpu_o3d.py holds them: equal, 1e-12, 1e-9, 1e-9."""
    c, tr = oc.icp_case(name), oc.oracle_trace(name)
    T, f, r, it = _icp(c)
    dT = np.abs(T - tr['T']).max()
    report(FILE, f'icp oracle    {name:28s} N0={len(c["src"]):6d} N1={len(c["dst"]):5d} iterations {it:2d} / {tr["iterations"]:2d}  matches '
                 f'{round(f * len(c["src"])):6d}  |T-oracle| {dT:.1e} of 1e-9  |rmse-oracle| {abs(r - tr["rmse"]):.1e} of 1e-9')
    assert it == tr['iterations']
    if name.startswith('criteria:'):
        assert it == oc.CRITERIA_ITERATIONS[name.partition(':')[2]]
    assert abs(f - tr['fitness']) < 1e-12 and abs(r - tr['rmse']) < 1e-9
    np.testing.assert_allclose(T, tr['T'], atol=1e-9)
    np.testing.assert_array_equal(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize('name', oc.EXACT_CASES)
def test_icp_one_step_within_bound(name):
    """One iteration from `init`: T = umeyama(matched pairs) @ init, the pairs by brute force over the finite rows, the
    Umeyama exact; R and t within bound_T.  The fitness after the step counts the matches over ALL N0 rows."""
    c = oc.icp_case(name)
    with np.errstate(invalid='ignore'):
        P = oc.placed(c)
    nn = oc.brute(name)
    ok = nn.idx >= 0
    Pm, Qm = P[ok], c['dst'].astype(np.float64)[nn.idx[ok]]
    ex = ref.umeyama_exact(Pm, Qm)
    d8 = c['dst'].astype(np.float64)
    corner = d8[np.isfinite(d8).all(1)].min(0)
    init = np.eye(4) if c['init'] is None else c['init']
    nb = ref.n_blocks(len(c['src']))
    T, f, r, it = _icp(c, max_iter=1)
    ratio, eR, bR, et, bt = ref.check_T(T, Pm, Qm, nb, corner, left=init, exact=ex)
    own = ref.check_T(o3.umeyama(Pm, Qm) @ init, Pm, Qm, nb, corner, left=init, exact=ex)
    report(FILE, f'icp one step  {name:28s} N0={len(c["src"]):6d} matches {int(ok.sum()):6d}  R: |dev-exact| {eR:.1e} bound {bR:.1e}   '
                 f't: |dev-exact| {et:.1e} bound {bt:.1e}   ratio {ratio:.2e}   centred f64 oracle: R {own[1]:.1e} t {own[3]:.1e}')
    assert it == 1 and np.isfinite(T).all()
    assert ratio <= 1, (name, eR, bR, et, bt)
    if len(c['src']) <= 5000:     # (the 65537-point case: its whole run is held to the oracle's fitness above)
        with np.errstate(invalid='ignore'):
            after = ref.nearest_bruteforce(c['src'].astype(np.float64) @ T[:3, :3].T + T[:3, 3], c['dst'], c['max_dist'])
        assert f == int((after.idx >= 0).sum()) / len(c['src'])


def test_icp_non_finite_rows_take_no_part():
    """NaN / +inf / -inf rows in both clouds (first row, last row, a partial wave): the run equals the run on the clouds
    without those rows -- same iterations, same matches (the fitness still divides by all N0 rows), T and rmse to the
    suite's 1e-9."""
    a, b = oc.icp_case('non_finite'), oc.icp_case('non_finite_clean')
    Ta, fa, ra, ita = _icp(a)
    Tb, fb, rb, itb = _icp(b)
    report(FILE, f'icp non-finite rows: iterations {ita} / {itb}  matches {round(fa * 300)} / {round(fb * 297)}  |dT| {np.abs(Ta - Tb).max():.1e}')
    assert len(a['src']) == 300 and len(b['src']) == 297
    assert ita == itb and abs(fa * 300 - fb * 297) < 1e-9 and fb > 0.9
    assert abs(ra - rb) < 1e-9
    np.testing.assert_allclose(Ta, Tb, atol=1e-9)


@pytest.mark.parametrize('name', oc.RANK1_CASES)
def test_icp_rank_one_update_is_a_rotation(name):
    """Two distinct matched target points: the covariance has rank 1 and the rotation is not unique.  What is pinned: T is
    finite, a rotation, and moves the matched pairs as close together as the oracle's T does."""
    c = oc.icp_case(name)
    P = oc.placed(c)
    nn = oc.brute(name)
    ok = nn.idx >= 0
    Pm, Qm = P[ok], c['dst'].astype(np.float64)[nn.idx[ok]]
    T, f, r, it = _icp(c)
    To = o3.icp_point_to_point(c['src'], c['dst'], c['max_dist'], init=c['init'], **c['kw'])[0]

    def residual(T):
        return float(np.sqrt((((Pm @ T[:3, :3].T + T[:3, 3]) - Qm) ** 2).sum(1).mean()))
    report(FILE, f'icp rank 1    {name:28s} matches {int(ok.sum()):4d}  residual {residual(T):.3e}  oracle {residual(To):.3e}  |T-oracle| '
                 f'{np.abs(T - To).max():.1e} (unpinned)')
    assert it == 1
    _is_rotation(T)
    assert abs(residual(T) - residual(To)) < 1e-12


def test_icp_ties_do_not_depend_on_the_row_order():
    """8 exactly equidistant target points per source point: the same bits from two runs, from the target with its rows
    reversed and with its rows permuted; every evaluation's fitness is the brute-force one."""
    src, dst, rev, perm = oc.ties()
    c = dict(src=src, dst=dst, max_dist=oc.MAX_DIST, init=None, kw={})
    runs = [_icp(c, max_iter=2), _icp(c, max_iter=2), _icp(c, dst=rev, max_iter=2), _icp(c, dst=perm, max_iter=2)]
    for k, (T, f, r, it) in enumerate(runs):
        report(FILE, f'icp ties      run {k} ({("first", "again", "reversed", "permuted")[k]:8s}) iterations {it} fitness {f!r} rmse {r!r} '
                     f'|T-first| {np.abs(T - runs[0][0]).max():.1e}')
    for T, f, r, it in runs[1:]:
        assert np.array_equal(T, runs[0][0]) and (f, r, it) == runs[0][1:]
    for k in (0, 1, 2):
        T, f, _, it = _icp(c, max_iter=k) if k < 2 else runs[0]
        nn = ref.nearest_bruteforce(src.astype(np.float64) @ T[:3, :3].T + T[:3, 3], dst, oc.MAX_DIST)
        assert it == k and f == (nn.idx >= 0).sum() / len(src)


# ---- RANSAC -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', oc.TILE_SEEDS)
@pytest.mark.parametrize('n', oc.TILE_N)
def test_ransac_tile_edges(n, seed):
    """Below, on and above one LDS tile of 512 correspondences, and two tiles + 1: winner, count, rmse and T as
    test_ransac_matches_oracle_exactly holds them."""
    X, Y = oc.corr_problem(n)
    To, ho, co, ro = oc.ransac_oracle(n, 2000, seed)
    T, h, c, r = _ransac(X, Y, 2000, seed)
    report(FILE, f'ransac tile   N={n:5d} seed {seed:#x}: winner {h} / {ho} count {c} / {co} |rmse-oracle| {abs(r - ro):.1e} of 1e-6 '
                 f'|T-oracle| {np.abs(T - To).max():.1e} of 1e-9')
    assert (h, c) == (ho, co) and co >= 20
    assert abs(r - ro) < 1e-6
    np.testing.assert_allclose(T, To, atol=1e-9)


@pytest.mark.parametrize('n', oc.REPEAT_N)
def test_ransac_repeated_samples(n):
    """So few correspondences that most 4-samples repeat one: hypotheses of rank 2, 1 and 0, whose rotation LAPACK and
    the kernel need not agree on.  Properties of what the kernel returns, (a)-(e) below."""
    hyp, seed = 3000, 0
    X, Y = oc.repeat_problem(n)
    T, h, c, r = _ransac(X, Y, hyp, seed)
    nd, S = oc.distinct_samples(n, hyp, seed)
    _is_rotation(T)                                                               # (a)
    Xs, Ys = X[S[h]].astype(np.float64), Y[S[h]].astype(np.float64)
    ex = ref.umeyama_exact(Xs, Ys)
    line = f'ransac repeat N={n:3d}: winner {h} with {nd[h]} distinct samples, count {c}'
    if nd[h] >= 3 and ex.s[1] > 1e-6 * ex.s[0]:                                   # (b) rank >= 2: the rotation is unique
        ratio, eR, bR, et, bt = ref.check_T(T, Xs, Ys, 1)
        line += f'  R: |dev-exact| {eR:.1e} bound {bR:.1e}  t: {et:.1e} bound {bt:.1e}  ratio {ratio:.2e}'
        assert ratio <= 1, (eR, bR, et, bt)
    report(FILE, line)
    thr2 = np.float32(np.float32(oc.RS_THR) * np.float32(oc.RS_THR))
    cc, err = ref.consensus(T, X, Y, thr2)                                        # (c)
    assert c == cc and r == (float(np.sqrt(err / cc)) if cc else 0.0)
    same = np.nonzero((S == S[h]).all(1))[0]                                      # (d) third key: the lowest index wins
    assert h == same[0], (h, same[:5])
    assert c >= oc.repeat_best_distinct(n, hyp, seed)                             # (e)
    assert 0 <= h < hyp and c >= 2


def test_ransac_non_finite_correspondences():
    """NaN and infinite coordinates among the correspondences: a hypothesis that samples one counts no inlier, such a
    row is nobody's inlier, and the result is the oracle's under that rule."""
    X, Y, To, ho, co, ro = oc.ransac_non_finite()
    T, h, c, r = _ransac(X, Y, 2000, 0)
    report(FILE, f'ransac non-finite: winner {h} / {ho} count {c} / {co} |T-oracle| {np.abs(T - To).max():.1e} of 1e-9')
    _is_rotation(T)
    with np.errstate(invalid='ignore', over='ignore'):
        cc, err = ref.consensus(T, X, Y, np.float32(np.float32(oc.RS_THR) * np.float32(oc.RS_THR)))
    assert c == cc and r == float(np.sqrt(err / cc))
    assert (h, c) == (ho, co) and abs(r - ro) < 1e-6
    np.testing.assert_allclose(T, To, atol=1e-9)
