"""Non-chaotic checks of the registration kernel's sums (csrc/reg.hip) against an f64 evaluation of the reference formulas
on the same f32 inputs, written with the implementation as a CALLABLE: tests/test_gpu_reg_clusters.py passes the HIP entry
points, tests/test_reg_checks_cpu.py passes the f32 oracle, a CPU model of the kernel's arithmetic and deliberately broken
variants of that model (which the checks must reject).

What is fixed HERE, not read from the code under test: the size grid, the cluster table and the chunk-ownership rule
(member j of a cluster of CL owns the 256-row chunks with chunk % CL == j), all three as documented in reg.hip's header.

Bounds (u = eps32 / 2 is one f32 rounding; every bound is computed in f64 from the inputs, none from an implementation):

PROCRUSTES, R.  The kernel adds 17 sums in f64, takes the 3x3 SVD in f64 and rounds R to f32 once.
  * rounding of R: entries |R| <= 1, so at most eps32 = 2^-23 per entry (half of that for entries above 0.5);
  * f64 summation: a thread adds at most ceil(n / 256) terms, then 6 shuffle steps, 4 waves, <= 8 members:
    D = ceil(n / 256) + 18 additions deep, whatever the cluster size, so every raw sum carries <= D eps64 sum|terms|; the
    covariance is the raw second moment minus (2 - sn) my mx^T (8 more f64 operations on quantities of the same size), i.e.
    dS <= (D + 8) eps64 raw,  raw = max_ab sum_i |wn_i y_ia x_ib| + 2 max|my| max|mx|  (the cancellation of a cloud far
    from the origin is IN this term: raw ~ 1e6 for a centroid of 1e3, the covariance ~ 1);
  * conditioning of the rotation (polar factor, real square case): |dR|_F <= 2 |dS|_F / gap with gap = s2 + sg s3, sg the
    sign of det(U) det(V) (s2 - s3 for a reflected covariance), |dS|_F <= 3 max|dS|; the same for the f64 yardstick's own
    LAPACK SVD, 1e-15 s1 / gap.
  bound_R = eps32 + (6 (D + 8) eps64 raw + 1e-15 s1) / gap.   Where gap < 1e-3 s1 (or on request) the project's criterion
  |impl - f64| <= 1.5 |f32 oracle - f64| is admitted as well, with bound_R as its floor.
PROCRUSTES, t = my - R mx in f32 from the f32-rounded R: two conversions and a multiplication per product (3 u |R||mx|), two
  additions (2 u |R||mx|), the conversion of my (u |my|) and the subtraction (u (|my| + |R||mx|)): <= 6 u = 3 eps32 times
  (|my| + |R||mx|), plus what R's own deviation moves: bound_t = 3 eps32 (|my| + |R||mx|) + dR_allowed sum|mx|.

LOSS AND GRADIENT at given parameters (`lossgrad_terms`).  Per row, in f32: p = R x + t, r = (p - y) / q, s = r.r,
  (per, dps) = SmoothL1, wk = w dps 2 / q, g = wk r, G = g x^T; summed in f64; divided by w1 and rounded to f32; the six
  rotation parameters by the f32 backward of ortho2rotation applied to G.
  * after r: division by q (1), s (3 products, 2 sums), sqrt + division or the 0.5 branch (2), wk (3), g (1), g x (1),
    per w (1) -- at most 12 roundings on any path -- plus w1 = f32(sum w) and the final f32 rounding: 14 u = 7 eps32,
    taken as C_TERM = 8;
  * before r: p is three products and three sums (6 u (|R||x| + |t|)) of an R whose entries come out of ~8 f32 operations
    on unit vectors (4 eps32 each): dp_i <= eps32 (3 (|R||x_i| + |t|) + 4 |x_i|_1) per component, and p - y CANCELS: the
    term of row i moves by at most 2 |dp_i| / |r_i q| of itself (linear in r below the knee, r / |r| above it, the loss
    term r.r or |r|);
  floor_k = eps32 sum_i |term_ik| (C_TERM + 2 |dp_i| / |p_i - y_i|) / w1   for the loss, the translation and G, and for the
  rotation parameters |J|^T floor_G + C_BACK eps32 |G-terms|_F, C_BACK = 32: the backward is ~30 f32 operations with O(1)
  coefficients on the entries of G.  Rows whose s is within 1e-5 of the knee s = 1 may take either branch (as in
  test_smooth_l1_hip_matches_reference): the difference of the two branches is added for those rows, and there may be at
  most NEAR_KNEE_CAP of them.  Criterion per component: |impl - f64| <= max(1.5 |f32 oracle - f64|, floor).
"""
import os

import numpy as np
import torch

from oracle import registration as oreg

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
CHUNK = 256
# reg.hip's header: 1, 2, 4 or 8 workgroups per pair by the pair's row count alone
CLUSTER_TABLE = ((16384, 8), (8192, 4), (4096, 2), (0, 1))
SMALL = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
THRESHOLDS = (4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385)
INTERIOR = (6000, 12000, 30000)      # 12000: 47 chunks over 4 members, the last one partial
GRID = SMALL + THRESHOLDS + INTERIOR
CLUSTERED = tuple(n for n in GRID if n >= 4096)
PATTERNS = ('a', 'b', 'c0', 'cL', 'd', 'e', 'f')
C_TERM, C_BACK, NEAR_KNEE_CAP = 8.0, 32.0, 3
Q = 0.1


def cluster_size(n):
    return next(cl for lo, cl in CLUSTER_TABLE if n >= lo)


def member_of_row(n):
    """Owner of every row: chunk % CL."""
    return (np.arange(n) // CHUNK) % cluster_size(n)


def report(name, line):
    print(line)
    rep = os.environ.get('DGR_PARITY_REPORT')
    if rep:
        os.makedirs(rep, exist_ok=True)
        with open(os.path.join(rep, name), 'a') as f:
            f.write(line + '\n')


# ---- inputs ---------------------------------------------------------------------------------------------------------
ROT_GT = oreg.rot6d_to_matrix(torch.tensor([[0.8, -0.5, 0.3, 0.4, 0.9, 0.1]], dtype=torch.float64))[0].numpy()
T_GT = np.array([0.3, -0.2, 0.1])


def geometry(n, offset=False, seed=0):
    """n correspondences, ~70 % outliers, in random order; the last row is always an inlier.  `offset`: both clouds about 1e3
    from the origin with a spread of about 1."""
    rng = np.random.default_rng(1000 * seed + n)
    spread = 1.0 if offset else 2.0
    X = rng.uniform(-spread, spread, (n, 3))
    Y = X @ ROT_GT.T + T_GT + rng.normal(scale=0.02, size=(n, 3))
    out = rng.random(n) < 0.7
    out[-1] = False
    Y[out] = rng.uniform(-1.5 * spread, 1.5 * spread, (int(out.sum()), 3))
    if offset:
        X = X + np.array([1000.0, -900.0, 1100.0])
        Y = Y + np.array([-950.0, 1050.0, 1000.0])
    return X.astype(np.float32), Y.astype(np.float32), out


def weights(pattern, n, outlier, seed=0):
    """Weight patterns of the issue; None where the pattern does not exist at this size."""
    rng = np.random.default_rng(77 * seed + n)
    w = np.where(outlier, rng.uniform(0, 0.2, n), rng.uniform(0.5, 1.0, n)).astype(np.float32)
    w[w < 0.05] = 0                                           # (a) pipeline-like
    cl = cluster_size(n)
    if pattern == 'a':
        return w
    if pattern == 'b':
        return np.ones(n, np.float32)
    if pattern in ('c0', 'cL'):                               # (c) one member without a surviving row
        if cl == 1:
            return None
        w[member_of_row(n) == (0 if pattern == 'c0' else cl - 1)] = 0
        return w
    if pattern == 'd':                                        # (d) one survivor per chunk
        keep = np.zeros(n, bool)
        for c0 in range(0, n, CHUNK):
            keep[c0 + int(rng.integers(0, min(CHUNK, n - c0)))] = True
        return np.where(keep, np.maximum(w, np.float32(0.3)), np.float32(0)).astype(np.float32)
    if pattern == 'e':                                        # (e) the final (partial) chunk + 8 rows elsewhere
        last = (n - 1) // CHUNK * CHUNK
        keep = np.arange(n) >= last
        keep[np.linspace(0, n - 1, 8).astype(int)] = True
        return np.where(keep, np.maximum(w, np.float32(0.3)), np.float32(0)).astype(np.float32)
    if pattern == 'f':                                        # (f) signed: every 9th surviving row negative
        nz = np.nonzero(w)[0][::9]
        w[nz] = -w[nz]
        return w
    raise ValueError(pattern)


def poses(X, Y, w):
    """The two parameter vectors of the loss/gradient check: the f64 Procrustes estimate turned by about 1 degree and moved
    by 2 cm (most inliers below the knee), and a far pose (most rows above it).  rot6d + trans, exact in f32."""
    if np.count_nonzero(w) >= 4:
        R, t = oreg.weighted_procrustes(X, Y, w, dtype=torch.float64)
        R, t = R.numpy(), t.numpy().reshape(3)
    else:
        R, t = ROT_GT, T_GT
    a = np.deg2rad(1.0)
    dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    near = np.concatenate([(dR @ R)[:, 0], (dR @ R)[:, 1], t + [0.02, -0.015, 0.01]])
    far = np.concatenate([R[:, 2], R[:, 0] + 0.2 * R[:, 1], t + [0.8, 0.5, -0.6]])
    return {'near': near.astype(np.float32).astype(np.float64), 'far': far.astype(np.float32).astype(np.float64)}


# ---- Procrustes -----------------------------------------------------------------------------------------------------
def procrustes_bounds(X, Y, w):
    """(R8, t8, bound_R without the fallback, gap / s1, mx, my) of the f64 evaluation; see the module docstring."""
    X8, Y8, w8 = (np.asarray(a, np.float32).astype(np.float64) for a in (X, Y, w))
    w8 = w8.reshape(-1, 1)
    n = len(X8)
    wn = w8 / (np.abs(w8).sum() + EPS32)
    mx, my = (wn * X8).sum(0), (wn * Y8).sum(0)
    S = (Y8 - my).T @ (wn * (X8 - mx))
    U, s, Vt = np.linalg.svd(S)
    sg = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    gap = s[1] + sg * s[2]
    raw = float(((np.abs(wn) * np.abs(Y8)).T @ np.abs(X8)).max() + 2 * np.abs(my).max() * np.abs(mx).max())
    D = -(-n // CHUNK) + 18
    R8, t8 = oreg.weighted_procrustes(X, Y, w, dtype=torch.float64)
    bound = EPS32 + (6 * (D + 8) * EPS64 * raw + 1e-15 * s[0]) / max(gap, 1e-300)
    return R8.numpy(), t8.numpy().reshape(3), bound, gap / max(s[0], 1e-300), mx, my


def check_procrustes(impl, X, Y, w, tag='', strict=None, file='reg_procrustes_parity.txt'):
    """`impl(X, Y, w) -> (R [3,3], t [3])`.  Raises AssertionError when R or t is outside the bound.  `strict` (default:
    where gap >= 1e-3 s1): the derived bound alone; otherwise max(bound, 1.5 |f32 oracle - f64|)."""
    R8, t8, bR, relgap, mx, my = procrustes_bounds(X, Y, w)
    R4, t4 = oreg.weighted_procrustes(X, Y, w)
    R, t = impl(X, Y, w)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    eR, e32R = np.abs(R - R8).max(), np.abs(R4.numpy().astype(np.float64) - R8).max()
    et, e32t = np.abs(t - t8), np.abs(t4.numpy().astype(np.float64).reshape(3) - t8)
    if strict is None:
        strict = relgap >= 1e-3
    allowR = bR if strict else max(bR, 1.5 * e32R)
    bt = 3 * EPS32 * (np.abs(my) + np.abs(R8) @ np.abs(mx)) + allowR * np.abs(mx).sum()
    allowt = bt if strict else np.maximum(bt, 1.5 * e32t)
    report(file, f'procrustes {tag:34s} n={len(X):6d} gap/s1 {relgap:.1e} {"strict" if strict else "x1.5  "} R: |impl-f64| {eR:.1e} '
                 f'|f32-f64| {e32R:.1e} bound {bR:.1e}   t: |impl-f64| {et.max():.1e} |f32-f64| {e32t.max():.1e} bound {bt.max():.1e}')
    assert np.isfinite(R).all() and np.isfinite(t).all(), (tag, R, t)
    assert eR <= allowR, (tag, 'R', eR, allowR, e32R)
    assert (et <= allowt).all(), (tag, 't', et, allowt, e32t)
    if strict:   # t against the implementation's OWN R: the 3 eps32 bound without the slack R's deviation is given above
        own = np.abs(t - (my - R @ mx))
        assert (own <= 3 * EPS32 * (np.abs(my) + np.abs(R) @ np.abs(mx))).all(), (tag, 't vs own R', own)
    return eR, et.max()


# ---- loss and gradient ----------------------------------------------------------------------------------------------
def _rot(prm, dtype):
    return oreg.rot6d_to_matrix(torch.as_tensor(prm[:6], dtype=dtype).reshape(1, 6))[0]


def oracle_lossgrad(X, Y, w, prm, q, dtype=torch.float32):
    """The reference's loss and its autograd gradient w.r.t. (rot6d, trans) at `prm`."""
    Xt, Yt, wt = (torch.as_tensor(np.asarray(a, np.float32)).to(dtype) for a in (X, Y, w))
    wt = wt.reshape(-1, 1)
    p = torch.as_tensor(np.asarray(prm, np.float64)).to(dtype).requires_grad_(True)
    P = Xt @ oreg.rot6d_to_matrix(p[:6].reshape(1, 6))[0].t() + p[6:].reshape(1, 3)
    loss = oreg.smooth_l1_highdim(P, Yt, wt, wt.sum(), q)
    loss.backward()
    return float(loss.detach()), p.grad.double().numpy()


def lossgrad_terms(X, Y, w, prm, q):
    """f64: per-row terms [n, 13] of (loss, dL/dt [3], dL/dR [9]) BEFORE the division by w1, for both branches of the knee,
    the branch mask, s, and the relative sensitivity 2 |dp_i| / |p_i - y_i| (in units of eps32) of row i's terms to the rounding of p."""
    X8, Y8, w8 = (np.asarray(a, np.float32).astype(np.float64) for a in (X, Y, w))
    w8 = w8.reshape(-1)
    R = _rot(prm, torch.float64).numpy()
    t = np.asarray(prm[6:], np.float64)
    d = X8 @ R.T + t - Y8
    r = d / q
    s = (r * r).sum(1)

    def terms(quad):
        per = np.where(quad, 0.5 * s, 0.5 * (np.sqrt(s + EPS32) - 0.5))
        dps = np.where(quad, 0.5, 0.25 / np.sqrt(s + EPS32))
        g = (w8 * dps * 2 / q)[:, None] * r
        return np.concatenate([(per * w8)[:, None], g, (g[:, :, None] * X8[:, None, :]).reshape(-1, 9)], axis=1)
    quad = s < 1
    dp = 3 * (np.abs(X8) @ np.abs(R).T + np.abs(t)) + 4 * np.abs(X8).sum(1, keepdims=True)      # in units of eps32
    sens = 2 * np.linalg.norm(dp, axis=1) / np.maximum(np.linalg.norm(d, axis=1), 1e-300)
    return terms(quad), terms(~quad), quad, s, sens


def lossgrad_reference(X, Y, w, prm, q):
    """f64 loss + gradient [10] and the per-component floor [10] of the module docstring; also the near-knee row count."""
    T, Tother, quad, s, sens = lossgrad_terms(X, Y, w, prm, q)
    w1 = float(np.asarray(w, np.float32).astype(np.float64).sum())
    near = np.abs(s - 1) < 1e-5
    fl13 = (EPS32 * (np.abs(T) * (C_TERM + sens)[:, None]).sum(0) + np.abs(T - Tother)[near].sum(0)) / abs(w1)
    S13 = T.sum(0) / w1
    p6 = torch.as_tensor(np.asarray(prm[:6], np.float64))
    J = torch.autograd.functional.jacobian(lambda v: oreg.rot6d_to_matrix(v.reshape(1, 6))[0].reshape(-1), p6).numpy()  # [9, 6]
    sa = np.abs(T[:, 4:]).sum(0) / abs(w1)
    val = np.concatenate([[S13[0]], J.T @ S13[4:], S13[1:4]])
    floor = np.concatenate([[fl13[0]], np.abs(J).T @ fl13[4:] + C_BACK * EPS32 * np.linalg.norm(sa), fl13[1:4]])
    floor[1:] += EPS32 * np.abs(val[1:])       # the gradient is read back as m / 0.1f: one more f32 rounding
    return val, floor, int(near.sum())


def check_lossgrad(impl, X, Y, w, prm, q=Q, tag='', file='reg_lossgrad_parity.txt'):
    """`impl(X, Y, w, prm, q) -> (loss, grad [9])` at the f32 parameters `prm` (rot6d, trans).  Per component:
    |impl - f64| <= max(1.5 |f32 oracle - f64|, floor)."""
    val, floor, near = lossgrad_reference(X, Y, w, prm, q)
    l8, g8 = oracle_lossgrad(X, Y, w, prm, q, torch.float64)
    ref = np.concatenate([[l8], g8])
    # the term-wise evaluation IS the reference's formula: it must reproduce autograd in f64
    assert np.abs(val - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (tag, val, ref)
    assert near <= NEAR_KNEE_CAP, (tag, near)
    l4, g4 = oracle_lossgrad(X, Y, w, prm, q)
    e32 = np.abs(np.concatenate([[l4], g4]) - ref)
    li, gi = impl(X, Y, w, prm, q)
    got = np.concatenate([[float(li)], np.asarray(gi, np.float64).reshape(9)])
    err = np.abs(got - ref)
    allow = np.maximum(1.5 * e32, floor)
    k = int(np.argmax(err / allow))
    report(file, f'loss+grad  {tag:34s} n={len(X):6d} near-knee rows {near}  worst component {k}: |impl-f64| {err[k]:.2e} '
                 f'|f32-f64| {e32[k]:.2e} floor {floor[k]:.2e} (value {ref[k]:+.3e});  loss: {err[0]:.2e} {e32[0]:.2e} {floor[0]:.2e}')
    assert np.isfinite(got).all(), (tag, got)
    assert (err <= allow).all(), (tag, k, err, allow)
    return err, e32, floor


# ---- CPU model of the kernel's arithmetic, and its broken variants -----------------------------------------------------
MUTANTS = ('drop_last_partial_chunk', 'member_twice', 'member_left_out', 'member_total_in_f32', 'keep_w_gt_0')


def row_multiplier(mutant, n, w):
    """How often a row enters the sums under `mutant` (None: the mutant does not act through row counts / is the identity
    at this size).  The affected member is member 1 -- or the last one for `member_left_out`."""
    cl = cluster_size(n)
    m = np.ones(n)
    if mutant == 'drop_last_partial_chunk':
        if n % CHUNK == 0:
            return None
        m[n // CHUNK * CHUNK:] = 0
    elif mutant == 'member_twice':
        if cl == 1:
            return None
        m[member_of_row(n) == 1] = 2
    elif mutant == 'member_left_out':
        if cl == 1:
            return None
        m[member_of_row(n) == cl - 1] = 0
    elif mutant == 'keep_w_gt_0':
        m[np.asarray(w).reshape(-1) < 0] = 0
    else:
        return None
    return m


def model_procrustes(X, Y, w, mutant=None):
    """The kernel's pass 1 on the CPU: 17 sums per member in f64, added in member order, f64 SVD, R rounded to f32, t in f32."""
    X8, Y8, w8 = (np.asarray(a, np.float32).astype(np.float64) for a in (X, Y, w))
    w8 = w8.reshape(-1)
    n = len(X8)
    cl, own = cluster_size(n), member_of_row(n)
    mult = np.ones(n)
    if mutant in ('drop_last_partial_chunk', 'member_twice', 'member_left_out'):   # (the compaction does not feed pass 1)
        mult = row_multiplier(mutant, n, w8)
    S = np.zeros(17)
    for j in range(cl):
        k = own == j
        wj = w8[k] * mult[k]
        part = np.concatenate([[np.abs(wj).sum(), wj.sum()], (wj[:, None] * X8[k]).sum(0), (wj[:, None] * Y8[k]).sum(0),
                               ((wj[:, None] * Y8[k]).T @ X8[k]).reshape(-1)])
        if mutant == 'member_total_in_f32' and j == 1:
            part = part.astype(np.float32).astype(np.float64)
        S += part
    inv = 1.0 / (S[0] + EPS32)
    sn, mx, my = S[1] * inv, S[2:5] * inv, S[5:8] * inv
    Sxy = S[8:].reshape(3, 3) * inv - (2.0 - sn) * np.outer(my, mx)
    U, _, Vt = np.linalg.svd(Sxy)
    sg = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = (U @ np.diag([1, 1, sg]) @ Vt).astype(np.float32)
    t = my.astype(np.float32) - R @ mx.astype(np.float32)
    return R, t


def model_lossgrad(X, Y, w, prm, q, mutant=None):
    """The kernel's iteration on the CPU: per-row terms in f32, 13 sums in f64 (each row `row_multiplier` times), divided by
    w1 = f32(sum w) and rounded to f32, the rotation parameters through the f32 backward of ortho2rotation."""
    Xt, Yt = (torch.as_tensor(np.asarray(a, np.float32)) for a in (X, Y))
    wt = torch.as_tensor(np.asarray(w, np.float32)).reshape(-1)
    n = len(Xt)
    mult = row_multiplier(mutant, n, wt.numpy()) if mutant else None
    mult = torch.ones(n, dtype=torch.float64) if mult is None else torch.as_tensor(mult)
    qf = torch.tensor(q, dtype=torch.float32)
    p6 = torch.as_tensor(np.asarray(prm[:6], np.float32)).requires_grad_(True)
    R = oreg.rot6d_to_matrix(p6.reshape(1, 6))[0]
    Rd = R.detach()
    r = (Xt @ Rd.t() + torch.as_tensor(np.asarray(prm[6:], np.float32)) - Yt) / qf
    s = (r * r).sum(1)
    quad = s < 1
    rt = torch.sqrt(s + torch.tensor(EPS32, dtype=torch.float32))
    per = torch.where(quad, 0.5 * s, 0.5 * (rt - 0.5))
    dps = torch.where(quad, torch.full_like(s, 0.5), 0.25 / rt)
    g = (wt * dps * 2 / qf)[:, None] * r
    w1 = float(wt.double().sum().float())
    loss = float(((per * wt).double() * mult).sum() / w1)
    gt = ((g.double() * mult[:, None]).sum(0) / w1).float()
    G = (((g[:, :, None] * Xt[:, None, :]).double() * mult[:, None, None]).sum(0) / w1).float()
    R.backward(G)
    return np.float32(loss), np.concatenate([p6.grad.numpy(), gt.numpy()])
