"""References for the ICP and the safeguard RANSAC of csrc/o3d.hip that share no code with the kernels: an exact Umeyama
(rational means and covariance, one rounding, LAPACK SVD), a brute-force nearest neighbour, the f32 consensus of
oracle/open3d_reg.py, and the bound the device is held to.  Everything here is computed from the inputs."""
import collections
import math
from fractions import Fraction

import numpy as np

from oracle.open3d_reg import consensus  # noqa: F401  (the statement of the consensus lives with the oracle)

EPS64 = float(np.finfo(np.float64).eps)
ICP_THREADS = 256          # o3d.hip's header: rows per block of icp_step_kernel, threads of icp_solve_kernel

Exact = collections.namedtuple('Exact', 'T s sg gap mp mq')


def _ints(A):
    """Exact integers K and a power of two D with A == K / D (A: finite f64 values)."""
    fr = [Fraction(float(v)) for v in np.asarray(A, np.float64).reshape(-1)]
    D = max((f.denominator for f in fr), default=1)          # every denominator is a power of two
    K = np.array([f.numerator * (D // f.denominator) for f in fr], dtype=object).reshape(np.shape(A))
    return K, D


def _longdouble(fr):
    hi = float(fr)
    return np.longdouble(hi) + np.longdouble(float(fr - Fraction(hi)))


def exact_moments(P, Q):
    """(mp [3], mq [3], sigma [3][3]) as Fractions: the means and the centred covariance sum (q - mq)(p - mp)^T / n."""
    KP, DP = _ints(P)
    KQ, DQ = _ints(Q)
    n = len(KP)
    sp = [sum(KP[:, b]) for b in range(3)]
    sq = [sum(KQ[:, a]) for a in range(3)]
    mp = [Fraction(int(s), DP * n) for s in sp]
    mq = [Fraction(int(s), DQ * n) for s in sq]
    # n^2 D_P D_Q sigma_ab = n sum q_a p_b - (sum q_a)(sum p_b), in integers
    sigma = [[Fraction(int(n * sum(KQ[:, a] * KP[:, b]) - sq[a] * sp[b]), n * n * DP * DQ) for b in range(3)] for a in range(3)]
    return mp, mq, sigma


def umeyama_exact(P, Q):
    """Eigen::umeyama(P -> Q) without scaling from exact moments: the covariance is rounded ONCE to f64, the rotation is
    U diag(1, 1, sg) V^T of its LAPACK SVD (sg = sign of det U det V), t = mq - R mp in long double from the exact means.
    Own error in R: about 1e-15 s1 / gap, gap = s2 + sg s3."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    T = np.eye(4)
    if len(P) == 0:
        return Exact(T, np.zeros(3), 1.0, 0.0, np.zeros(3), np.zeros(3))
    mp, mq, sigma = exact_moments(P, Q)
    S = np.array([[float(v) for v in row] for row in sigma])
    U, s, Vt = np.linalg.svd(S)
    sg = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, sg]) @ Vt
    mpl, mql = np.array([_longdouble(v) for v in mp]), np.array([_longdouble(v) for v in mq])
    T[:3, :3] = R
    T[:3, 3] = (mql - R.astype(np.longdouble) @ mpl).astype(np.float64)
    return Exact(T, s, sg, float(s[1] + sg * s[2]), mpl.astype(np.float64), mql.astype(np.float64))


Nearest = collections.namedtuple('Nearest', 'idx d2 margin gap')


def nearest_bruteforce(P, dst, max_dist, chunk=512):
    """For every row of P the nearest finite row of dst within max_dist, in f64 over all pairs.  idx [n] (row of dst, -1:
    none, also for a non-finite row of P), d2 [n] of the nearest finite row (inf: none), margin [n] = |d2 - max_dist^2| /
    max_dist^2, gap [n] = (d2 of the second nearest - d2) / d2 of the second nearest (inf where there is no second)."""
    P, dst = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    rows = np.nonzero(np.isfinite(dst).all(1))[0]
    D = dst[rows]
    n, md2 = len(P), float(max_dist) * float(max_dist)
    idx, d2, gap = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    okp = np.isfinite(P).all(1)
    for i0 in range(0, n, chunk):
        sl = np.nonzero(okp[i0:i0 + chunk])[0] + i0
        if not len(sl) or not len(D):
            continue
        e = D[None, :, 0] - P[sl, None, 0]
        dd = e * e
        for ax in (1, 2):
            np.subtract(D[None, :, ax], P[sl, None, ax], out=e)
            dd += e * e
        j = np.argmin(dd, axis=1)
        d2[sl] = dd[np.arange(len(sl)), j]
        idx[sl] = rows[j]
        if len(D) > 1:
            dd[np.arange(len(sl)), j] = np.inf
            second = dd.min(1)
            gap[sl] = (second - d2[sl]) / np.maximum(second, 1e-300)
    margin = np.abs(d2 - md2) / md2
    idx[~(d2 <= md2)] = -1
    return Nearest(idx, d2, margin, gap)


def n_blocks(n_src):
    return -(-int(n_src) // ICP_THREADS)


def bound_T(P, Q, nblocks, origin=None, exact=None):
    """(bound_R, bound_t) for a device Umeyama of the pairs P -> Q whose 17 sums are added in f64 relative to `origin`
    (ICP: the minimum corner of the target's bounding box; None: absolute coordinates, RANSAC's 4-point solve).
      bound_R = (6 (D + 8) eps64 raw_c + 1e-15 s1) / gap,   D = 6 + 4 + ceil(nblocks / 256) + 8
    (6 shuffle steps, 4 waves, the strided pass and the 8 tree levels over the block partials; 8 more operations form the
    covariance; |dR|_F <= 2 |dS|_F / gap, |dS|_F <= 3 max|dS|; the yardstick's own SVD 1e-15 s1 / gap),
      raw_c = max_ab sum|q'_a p'_b| / n + 2 max|mq'| max|mp'|,
      bound_t = bound_R sum|mp'| + 4 eps64 (|mq| + |mp|)   (t = mq - R mp: products and sums of absolute coordinates)."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    ex = exact if exact is not None else umeyama_exact(P, Q)
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    Pp, Qp = P - o, Q - o
    n = len(P)
    mpp, mqp = ex.mp - o, ex.mq - o
    raw = float((np.abs(Qp).T @ np.abs(Pp)).max() / n + 2 * np.abs(mqp).max() * np.abs(mpp).max())
    D = 6 + 4 + math.ceil(nblocks / ICP_THREADS) + 8
    bR = (6 * (D + 8) * EPS64 * raw + 1e-15 * ex.s[0]) / max(ex.gap, 1e-300)
    bt = bR * np.abs(mpp).sum() + 4 * EPS64 * (np.linalg.norm(ex.mq) + np.linalg.norm(ex.mp))
    return bR, bt


def check_T(T, P, Q, nblocks, origin=None, left=None, exact=None):
    """Deviation of the device's T from umeyama_exact(P, Q) (@ left) as (ratio to the bound, eR, bR, et, bt)."""
    ex = exact if exact is not None else umeyama_exact(P, Q)
    bR, bt = bound_T(P, Q, nblocks, origin, ex)
    Tx = ex.T if left is None else (ex.T.astype(np.longdouble) @ np.asarray(left, np.longdouble)).astype(np.float64)
    eR, et = float(np.abs(T[:3, :3] - Tx[:3, :3]).max()), float(np.abs(T[:3, 3] - Tx[:3, 3]).max())
    return max(eR / bR, et / bt), eR, bR, et, bt
