"""The ICP and RANSAC edge cases the CPU and GPU tests of csrc/o3d.hip share, and their CPU references, each computed
once per session.  A case is a dict(src, dst, max_dist, init, kw); `kw` are the criteria of `icp_point_to_point` in the
oracle's spelling (ops_kw translates them)."""
import functools

import numpy as np

from oracle import open3d_reg as o3

MAX_DIST = 0.1
OFFSET_DIR = np.array([1.0, -0.9, 1.1])
OFFSETS = (0, 50, 1000)
CELL_CAP = 4 << 20          # o3d.hip's header / DESIGN.md 4.5: the grid's edge doubles until it has at most 4 M cells


def rot(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose_about(R, centre, shift):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = centre - R @ centre + shift
    return T


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def pair(seed, n_src, n_dst=3000, offset=0.0, spread=1.0, noise=0.01, flat=False):
    """A target of n_dst uniform points around offset * OFFSET_DIR, a source that is a noisy sample of it under a pose of
    0.3 rad about the cloud's centre, and an initial pose 0.01 rad / 2 cm away from the true one."""
    rng = np.random.default_rng(seed)
    c = offset * OFFSET_DIR
    dst = rng.uniform(-spread, spread, (n_dst, 3))
    if flat:
        dst[:, 2] = 0.5
    dst = (dst + c).astype(np.float32)
    pick = rng.integers(0, n_dst, n_src) if n_src > n_dst else rng.permutation(n_dst)[:n_src]
    T_gt = pose_about(rot(rng.standard_normal(3), 0.3), c, np.array([0.1, -0.2, 0.15]))
    moved = dst[pick].astype(np.float64) + rng.normal(0, noise, (n_src, 3))
    src = ((moved - T_gt[:3, 3]) @ T_gt[:3, :3]).astype(np.float32)
    init = pose_about(rot(rng.standard_normal(3), 0.01), c, np.array([0.02, -0.01, 0.015])) @ T_gt
    return src, dst, init


def _case(src, dst, init=None, max_dist=MAX_DIST, **kw):
    return _freeze(dict(src=np.ascontiguousarray(src, np.float32), dst=np.ascontiguousarray(dst, np.float32),
                        max_dist=max_dist, init=init, kw=kw))


SIZES_N0 = (1, 63, 64, 65, 255, 256, 257, 65537)
CRITERIA = {'max_iter_0': dict(max_iter=0), 'max_iter_1': dict(max_iter=1), 'max_iter_2': dict(max_iter=2),
            'never_converged': dict(max_iter=6, rel_fitness=0.0, rel_rmse=0.0),
            'at_once_converged': dict(max_iter=6, rel_fitness=1e9, rel_rmse=1e9)}
# what the criteria cases must run, from Registration.cpp's loop alone
CRITERIA_ITERATIONS = {'max_iter_0': 0, 'max_iter_1': 1, 'max_iter_2': 2, 'never_converged': 6, 'at_once_converged': 1}


def _few_matches(k):
    """k source points 2 cm from a target point each, 20 more half a unit outside the target's box."""
    rng = np.random.default_rng(40 + k)
    _, dst, _ = pair(7, 10)
    near = dst[rng.permutation(len(dst))[:k]].astype(np.float64) + rng.normal(0, 0.012, (k, 3))
    far = rng.uniform(-1, 1, (20, 3))
    far[:, rng.integers(0, 3)] = 1.5
    far[::2] *= -1
    return _case(np.concatenate([far[:7], near, far[7:]]), dst)


def _negative_faces():
    """The raw source lies 50 units below the grid on every axis and `init` brings it back; 10 more points per face lie
    4 cm outside that face of the target's box, next to the target points closest to it."""
    src, dst, init = pair(11, 500)
    d8 = dst.astype(np.float64)
    lo, hi = d8.min(0), d8.max(0)
    extra = []
    for ax in range(3):
        for side, edge in ((0, lo), (1, hi)):
            order = np.argsort(d8[:, ax])
            p = d8[order[:10] if side == 0 else order[-10:]].copy()
            p[:, ax] = edge[ax] + (-0.04 if side == 0 else 0.04)
            extra.append(p)
    extra = np.concatenate(extra)
    placed = np.concatenate([src.astype(np.float64) @ init[:3, :3].T + init[:3, 3], extra])
    shift = np.eye(4)
    shift[:3, 3] = 50.0
    return _case(placed - 50.0, dst, shift)


def _mirror():
    """A thin slab (|z| < 0.01, xy spacing above 0.25) and its mirror image in z: every point's nearest neighbour is its
    own image, and the matched covariance has a negative determinant."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing='ij'), -1).reshape(-1, 2) * 0.3
    src = np.concatenate([g + rng.uniform(-0.02, 0.02, g.shape), rng.uniform(-0.01, 0.01, (len(g), 1))], 1).astype(np.float32)
    dst = src * np.array([1, 1, -1], np.float32)
    return _case(src, dst[rng.permutation(len(dst))], max_iter=1)


def _non_finite(clean):
    src, dst, init = pair(13, 300)
    bad = np.array([[np.nan, np.nan, np.nan], [np.inf, 0.1, 0.2], [0.3, -np.inf, 0.1]], np.float32)
    rows_s, rows_d = (0, 290, 299), (0, 2990, 2999)          # first row, a partial wave, last row
    if clean:
        return _case(np.delete(src, rows_s, 0), np.delete(dst, rows_d, 0), init)
    src, dst = src.copy(), dst.copy()
    src[list(rows_s)] = bad
    dst[list(rows_d)] = bad[::-1]
    return _case(src, dst, init)


@functools.lru_cache(maxsize=None)
def icp_case(name):
    kind, _, arg = name.partition(':')
    if kind == 'n0':
        return _case(*pair(20 + int(arg), int(arg)))
    if kind == 'n1':                                          # 300 source points around 1 or 2 target points
        rng = np.random.default_rng(30 + int(arg))
        dst = rng.uniform(-1, 1, (int(arg), 3)).astype(np.float32)
        src = dst[rng.integers(0, int(arg), 300)].astype(np.float64) + rng.normal(0, 0.02, (300, 3))
        return _case(src, dst, **({'max_iter': 1} if int(arg) == 2 else {}))
    if kind == 'cell_doubling':
        src, dst, init = pair(3, 1000, spread=20.0)
        return _case(src, dst, init)
    if kind == 'flat_axis':
        src, dst, init = pair(4, 1000, flat=True)
        return _case(src, dst, init)
    if kind == 'negative_far':
        src, dst, _ = pair(5, 500)
        return _case(src - np.float32(50.0), dst)
    if kind == 'negative_faces':
        return _negative_faces()
    if kind == 'non_finite':
        return _non_finite(clean=False)
    if kind == 'non_finite_clean':
        return _non_finite(clean=True)
    if kind == 'criteria':
        src, dst, init = pair(6, 1000)
        return _case(src, dst, init, **CRITERIA[arg])
    if kind == 'few_matches':
        c = _few_matches(int(arg))
        return _case(c['src'], c['dst'], max_iter=1) if int(arg) == 2 else c
    if kind == 'mirror':
        return _mirror()
    if kind in ('one_step', 'full_run'):
        src, dst, init = pair(8, 2500, offset=float(arg))
        return _case(src, dst, init, **({'max_iter': 1} if kind == 'one_step' else {}))
    raise KeyError(name)


# compared with the KD-tree oracle: iteration count, fitness, rmse and T
ORACLE_CASES = tuple(f'n0:{n}' for n in SIZES_N0) + ('n1:1', 'cell_doubling', 'flat_axis', 'negative_far', 'negative_faces',
                                                      'non_finite_clean') + tuple(f'criteria:{k}' for k in CRITERIA) + \
    ('few_matches:0', 'few_matches:1', 'few_matches:3') + tuple(f'full_run:{o}' for o in OFFSETS)
# one step from `init`, compared with umeyama_exact of the brute-force matches within bound_T
EXACT_CASES = ('mirror', 'non_finite', 'n0:65537', 'n0:257', 'n0:63') + tuple(f'one_step:{o}' for o in OFFSETS)
# the rotation is not unique (two distinct matched target points): properties only
RANK1_CASES = ('few_matches:2', 'n1:2')


def ops_kw(case):
    names = {'max_iter': 'max_iter', 'rel_fitness': 'relative_fitness', 'rel_rmse': 'relative_rmse'}
    return {names[k]: v for k, v in case['kw'].items()}


def placed(case):
    """The source under `init`, in f64."""
    T = np.eye(4) if case['init'] is None else np.asarray(case['init'], np.float64)
    return case['src'].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


@functools.lru_cache(maxsize=None)
def brute(name):
    """Brute-force matches of a case's source under `init` (tests/o3d_ref.py: nearest_bruteforce), once per session."""
    import o3d_ref
    c = icp_case(name)
    with np.errstate(invalid='ignore'):
        return o3d_ref.nearest_bruteforce(placed(c), c['dst'], c['max_dist'])


def layout(dst, max_dist, cell_cap=CELL_CAP):
    """The grid rule of DESIGN.md 4.5: (cell edge, dims [3], doublings) over the finite rows of dst."""
    d = np.asarray(dst, np.float32)
    d = d[np.isfinite(d).all(1)].astype(np.float64)
    lo, hi = d.min(0), d.max(0)
    cell, doublings = float(max_dist), 0
    while np.prod(np.floor((hi - lo) / cell) + 1.0) > cell_cap:
        cell *= 2.0
        doublings += 1
    return cell, (np.floor((hi - lo) / cell) + 1.0).astype(np.int64), doublings


@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    """The oracle's run of a case, statement by statement as `o3.icp_point_to_point`, with what the preconditions need:
    dict(T, fitness, rmse, iterations, margin, gap, matches) -- the smallest relative distance of any match from
    max_dist^2 and the smallest relative gap between nearest and second nearest over ALL evaluations, the match count of
    each evaluation."""
    from scipy.spatial import cKDTree
    c = icp_case(name)
    kw = dict(max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6)
    kw.update(c['kw'])
    src, dst = c['src'].astype(np.float64), c['dst'].astype(np.float64)
    T = np.eye(4) if c['init'] is None else np.asarray(c['init'], np.float64).copy()
    P = src @ T[:3, :3].T + T[:3, 3]
    tree = cKDTree(dst)
    md2 = c['max_dist'] ** 2
    log = dict(margin=np.inf, gap=np.inf, matches=[])

    def evaluate(P):
        d, _ = tree.query(P, k=2) if len(dst) > 1 else (np.stack([tree.query(P)[0], np.full(len(P), np.inf)], 1), None)
        d2a, d2b = d[:, 0] ** 2, d[:, 1] ** 2
        log['margin'] = min(log['margin'], float(np.min(np.abs(d2a - md2) / md2)))
        near = d2a < 4 * md2                                       # a tie far outside the radius decides nothing
        if near.any() and len(dst) > 1:
            log['gap'] = min(log['gap'], float(np.min((d2b[near] - d2a[near]) / d2b[near])))
        out = o3._evaluate_icp(P, tree, dst, c['max_dist'])
        log['matches'].append(len(out[0]))
        return out
    ci, cj, fit, rmse = evaluate(P)
    it = 0
    for it in range(1, kw['max_iter'] + 1):
        upd = o3.umeyama(P[ci], dst[cj])
        T = upd @ T
        P = P @ upd[:3, :3].T + upd[:3, 3]
        pf, pr = fit, rmse
        ci, cj, fit, rmse = evaluate(P)
        if abs(pf - fit) < kw['rel_fitness'] and abs(pr - rmse) < kw['rel_rmse']:
            break
    T.setflags(write=False)
    return dict(T=T, fitness=fit, rmse=rmse, iterations=it, margin=log['margin'], gap=log['gap'], matches=tuple(log['matches']))


# ---- determinism ------------------------------------------------------------------------------------------------------
TIE_SCALE = 13.0 / 256       # 0.05 to 8 bits: lattice and cell centres are exact in f32, so the 8 distances tie EXACTLY in f64


@functools.lru_cache(maxsize=None)
def ties():
    """Target: a 12^3 integer lattice times TIE_SCALE; source: the 11^3 cell centres.  (src, dst, reversed, permuted)."""
    k = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing='ij'), -1).reshape(-1, 3)
    dst = (k * TIE_SCALE).astype(np.float32)
    src = ((k[(k < 11).all(1)] + 0.5) * TIE_SCALE).astype(np.float32)
    perm = np.random.default_rng(0).permutation(len(dst))
    out = (src, dst, np.ascontiguousarray(dst[::-1]), np.ascontiguousarray(dst[perm]))
    for a in out:
        a.setflags(write=False)
    return out


# ---- RANSAC -----------------------------------------------------------------------------------------------------------
TILE_N = (511, 512, 513, 1025)
TILE_SEEDS = (0, 1, 0xfffffff1)
REPEAT_N = (4, 5, 63)
RS_THR = 0.1


@functools.lru_cache(maxsize=None)
def corr_problem(n, outlier_frac=0.7, seed=None):
    """n correspondences X -> Y = R X + t + 5 mm noise, `outlier_frac` of them replaced by uniform points."""
    rng = np.random.default_rng(100 + n if seed is None else seed)
    X = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    R, t = rot(rng.standard_normal(3), rng.uniform(0, np.pi)), rng.uniform(-1, 1, 3)
    Y = (X @ R.T + t + rng.normal(0, 0.005, (n, 3))).astype(np.float32)
    out = rng.random(n) < outlier_frac
    Y[out] = rng.uniform(-3, 3, (int(out.sum()), 3)).astype(np.float32)
    for a in (X, Y):
        a.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def ransac_oracle(n, hyp, seed):
    X, Y = corr_problem(n)
    return o3.ransac_correspondence(X, Y, RS_THR, hyp, seed=seed)


def distinct_samples(n, hyp, seed):
    """Number of distinct correspondences among the 4 draws of every hypothesis."""
    S = o3.ransac_samples(seed, 0, hyp, n)
    return np.array([len(set(r)) for r in S.tolist()]), S


def repeat_problem(n):
    """Noisy inliers only at 4 and 5 correspondences (every 4-subset of 5 with two outliers holds one), 30 % outliers at 63."""
    return corr_problem(n, 0.3 if n > 5 else 0.0, seed=200 + n)


@functools.lru_cache(maxsize=None)
def repeat_best_distinct(n, hyp, seed):
    """Largest consensus count among the oracle's hypotheses whose 4 samples are distinct."""
    X, Y = repeat_problem(n)
    nd, S = distinct_samples(n, hyp, seed)
    thr2 = np.float32(np.float32(RS_THR) * np.float32(RS_THR))
    X8, Y8 = X.astype(np.float64), Y.astype(np.float64)
    seen, best = set(), -1
    for h in np.nonzero(nd == 4)[0]:
        key = tuple(S[h])
        if key not in seen:
            seen.add(key)
            best = max(best, o3.consensus(o3.umeyama(X8[S[h]], Y8[S[h]]), X, Y, thr2)[0])
    return best


NF_ROWS = {'X': ((0, np.nan), (300, -np.inf)), 'Y': ((599, np.inf), (17, np.nan))}


@functools.lru_cache(maxsize=None)
def ransac_non_finite(hyp=2000, seed=0):
    """600 correspondences, four of them with a NaN or an infinite coordinate, and the oracle's run in which a hypothesis
    that samples one of those rows counts no inlier: (X, Y, T, h, count, rmse)."""
    X, Y = (a.copy() for a in corr_problem(600, 0.6))
    for name, A in (('X', X), ('Y', Y)):
        for row, v in NF_ROWS[name]:
            A[row, row % 3] = v
    bad = ~(np.isfinite(X).all(1) & np.isfinite(Y).all(1))
    thr2 = np.float32(np.float32(RS_THR) * np.float32(RS_THR))
    S = o3.ransac_samples(seed, 0, hyp, len(X))
    X8, Y8 = X.astype(np.float64), Y.astype(np.float64)
    best = (-1, np.inf, -1, np.eye(4))
    with np.errstate(invalid='ignore', over='ignore'):
        for h in range(hyp):
            if bad[S[h]].any():
                c, err, T = 0, 0.0, None
            else:
                T = o3.umeyama(X8[S[h]], Y8[S[h]])
                c, err = o3.consensus(T, X, Y, thr2)
            if c > best[0] or (c == best[0] and err < best[1]):
                best = (c, err, h, T)
    c, err, h, T = best
    for a in (X, Y):
        a.setflags(write=False)
    return X, Y, T, h, c, (float(np.sqrt(err / c)) if c > 0 else 0.0)
