"""Seeded case builders of the batched k-NN route tests (tests/test_gpu_knn_routes.py), checked on the CPU by
tests/test_knn_cases_cpu.py.  Pure numpy: nothing of the library is imported, the constants below restate
csrc/knn_common.h / knn_prefilter.h / knn.hip / knn_topk.hip and `emulate` restates the hi + lo bf16 split of
knn_pack_kernel and the three products the MFMA passes sum (d~' = nb - 2 (hi.hi + hi.lo + lo.hi), here in float64).

Every pair is a `Pair` with a `kind`:
  big        n1 in {1024, 1100, 1537}, n0 no multiple of 32: prefiltered, no fallback
  small      n1 in {5, 700, 1023} (one pair with n0 = 1): the brute-force route inside a mixed table
  k_gt_n1    n1 = 20: padding columns
  dup32/33   1100 references of which 32 / 33 consecutive rows are identical, 40 queries within 1e-4 of that row, every
             other reference (and query) deep in the opposite half-space: exactly KNN_SLOTS candidates / one more
  list64/65  as dup33 with 64 / 65 such queries: the last overflow list the 1-NN scan kernel takes / the first it leaves
  list64w/65w  the same beside 330 identical rows: the 32 slots then hold a tenth of the duplicates, so a listed query
             that nobody redoes returns a wrong row (with 33 duplicates the smallest row almost always has a slot and
             a dropped list changes no value)
  list256/257  a cluster of 2 * slots(32) + 1 = 1025 identical rows, 256 / 257 queries beside it: the same boundary of the
             top-k search (KNN_TOPK_SCAN_MAX), for every k at once
  fallback   one 1e20 / NaN / inf in one reference row: the pair's whole search redone by brute force
  aligned    the bound: see `aligned_pair`
Queries are redrawn until, outside the duplicate clusters, the first 33 float64 distances of every query are more than
2 * TIE_TOL apart: the GPU tests may then demand EQUAL indices instead of excusing differences as ties."""
import numpy as np

TIE_TOL = 2e-6          # the suite's tie tolerance (test_gpu_knn_reg.py, test_gpu_knn_topk.py)
KNN_TAU_C = 8e-5
KNN_SLOTS = 32
KNN_SCAN_MAX = 64
KNN_TOPK_SCAN_MAX = 256
KNN_MAXP = 32
KNN_MIN_REFS = 1024
KNN_ST = 4              # reference tiles per stage of the MFMA passes
TOP = 33                # float64 neighbours kept per query: the k = 32 comparison needs the 33rd
KS = (1, 2, 8, 32)


def topk_slots(k):
    K = 2
    while K < k:
        K *= 2
    return 512 if K >= 32 else 16 * K


class Pair:
    def __init__(self, kind, F0, F1, **meta):
        self.kind, self.F0, self.F1 = kind, np.ascontiguousarray(F0, np.float32), np.ascontiguousarray(F1, np.float32)
        self.cluster = meta.pop('cluster', None)      # (first, end) rows of the identical references
        self.near = meta.pop('near', None)            # query rows beside the cluster
        self.meta = meta

    @property
    def n0(self):
        return len(self.F0)

    @property
    def n1(self):
        return len(self.F1)

    @property
    def prefiltered(self):
        return self.n1 >= KNN_MIN_REFS


# ----------------------------------------------------------------------------------------------
# float64 reference and the emulated prefilter
# ----------------------------------------------------------------------------------------------
def d2_f64(F0, F1):
    """float64 squared distances [n0, n1]; references the f32 kernels never return (non-finite rows, distances beyond
    the f32 range) at +inf."""
    a, b = F0.astype(np.float64), F1.astype(np.float64)
    with np.errstate(all='ignore'):
        D = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
        D[~np.isfinite(D) | (D > 3e38)] = np.inf
        D[:, ~np.isfinite(F1).all(1)] = np.inf
    return np.maximum(D, 0.0)


def d2_f64_of(F0, F1, idx):
    """float64 squared distance of F0[i] to F1[idx[i, j]], by differences (exact to the last bits)."""
    with np.errstate(all='ignore'):
        D = ((F0.astype(np.float64)[:, None, :] - F1.astype(np.float64)[idx]) ** 2).sum(-1)
    D[~np.isfinite(D) | (D > 3e38)] = np.inf
    return D


def f64_topk(F0, F1, m=TOP):
    """(idx [n0, m'], D2 [n0, m']) of the m' = min(m, n1) nearest references in float64, equal distances by the
    smaller index (what the kernels' (distance bits, index) keys do with equal f32 distances)."""
    D = d2_f64(F0, F1)
    m = min(m, D.shape[1])
    idx = np.argsort(D, axis=1, kind='stable')[:, :m]
    return idx, d2_f64_of(F0, F1, idx)


def tie_free(idx, D, k, cluster=None, tol=TIE_TOL):
    """Rows whose first k + 1 float64 distances are pairwise more than tol apart -- gaps between two rows of the
    duplicate cluster excepted, where the expected order is the ascending row index.  [n0] bool."""
    m = min(k + 1, D.shape[1])
    with np.errstate(invalid='ignore'):
        ok = (D[:, 1:m] - D[:, :m - 1]) > tol
    ok |= np.isinf(D[:, 1:m])                        # exhausted: nothing finite left to tie with
    if cluster is not None:
        inc = (idx >= cluster[0]) & (idx < cluster[1])
        ok |= inc[:, 1:m] & inc[:, :m - 1]
    return ok.all(1)


def bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def split(x):
    """knn_pack_kernel: hi = bf16(x), lo = bf16(x - hi)."""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


def emulate(F0, F1):
    """(d~' [n0, n1] float64, na [n0], nb [n1], tau [n0]): the approximate distances of the MFMA passes less the query
    norm, the squared norms, and the bound's tau = KNN_TAU_C (na + max nb)."""
    qh, ql = (v.astype(np.float64) for v in split(F0))
    rh, rl = (v.astype(np.float64) for v in split(F1))
    na = (F0.astype(np.float64) ** 2).sum(1).astype(np.float32).astype(np.float64)
    nb = (F1.astype(np.float64) ** 2).sum(1).astype(np.float32).astype(np.float64)
    dp = nb[None, :] - 2.0 * (qh @ rh.T + ql @ rh.T + qh @ rl.T)
    return dp, na, nb, KNN_TAU_C * (na + nb.max())


def d2_f32_kernel(F0, F1, idx):
    """knn_d2 of the kernels for the listed references: two interleaved f32 fma chains, then one add (each fma: the
    exact square added in float64, rounded once to f32)."""
    a = F0.astype(np.float32)[:, None, :]
    b = F1.astype(np.float32)[idx]
    e = (a - b).astype(np.float32).astype(np.float64)
    d = [np.zeros(e.shape[:2], np.float32), np.zeros(e.shape[:2], np.float32)]
    for c in range(e.shape[2]):
        d[c & 1] = (e[..., c] * e[..., c] + d[c & 1].astype(np.float64)).astype(np.float32)
    return (d[0] + d[1]).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# random families
# ----------------------------------------------------------------------------------------------
def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def away(rng, n, c, depth=0.4, C=32):
    """n unit rows with x . c = -depth: deep in the half-space opposite to c."""
    g = rng.standard_normal((n, C))
    g -= (g @ c)[:, None] * c[None, :]
    g *= np.sqrt(1.0 - depth * depth) / np.linalg.norm(g, axis=1, keepdims=True)
    return (g - depth * c[None, :]).astype(np.float32)


def _settle(F0, F1, redraw, cluster=None, free=None):
    """Redraws the queries `redraw(rows)` may replace until every one of them is tie-free (2 * TIE_TOL) at TOP - 1."""
    for _ in range(50):
        idx, D = f64_topk(F0, F1)
        bad = ~tie_free(idx, D, TOP - 1, cluster, 2 * TIE_TOL)
        if free is not None:
            bad &= free
        if not bad.any():
            return F0
        F0[bad] = redraw(int(bad.sum()))
    raise RuntimeError('queries did not settle')


def random_pair(kind, seed, n0, n1, C=32):
    rng = np.random.default_rng(seed)
    F0, F1 = unit(rng.standard_normal((n0, C))), unit(rng.standard_normal((n1, C)))
    F0 = _settle(F0, F1, lambda n: unit(rng.standard_normal((n, C))))
    return Pair(kind, F0, F1)


def cluster_pair(kind, seed, dup, n_near, n_other, n1=1100, start=None):
    """`dup` identical consecutive reference rows c (from row `start`; the default makes the cluster cover the last,
    short stage of tiles), n_near queries within 1e-4 of c, n_other queries and all other references at x . c = -0.4."""
    rng = np.random.default_rng(seed)
    n_tiles = (n1 + 31) // 32
    if start is None:
        start = 20 + 2 * n_tiles
    c = unit(rng.standard_normal((1, 32)))[0].astype(np.float64)
    F1 = away(rng, n1, c)
    F1[start:start + dup] = c.astype(np.float32)
    n0 = n_near + n_other
    near = np.sort(rng.permutation(n0)[:n_near])
    F0 = away(rng, n0, c)
    u = rng.standard_normal((n_near, 32))
    F0[near] = unit(c[None, :] + 0.7e-4 * u / np.linalg.norm(u, axis=1, keepdims=True))
    free = np.ones(n0, bool)
    free[near] = False                                # the near queries stay: their ties are the cluster's
    F0 = _settle(F0, F1, lambda n: away(rng, n, c), (start, start + dup), free)
    return Pair(kind, F0, F1, cluster=(start, start + dup), near=near)


def fallback_pair(seed, value, n0=150, n1=1100):
    p = random_pair('fallback', seed, n0, n1)
    p.F1[7, 3] = value
    p.meta['value'] = value
    return p


# ----------------------------------------------------------------------------------------------
# the bound: aligned / opposed split residuals
# ----------------------------------------------------------------------------------------------
def pass1_stages(n_tiles, splits, sub=2):
    """Stages (groups of KNN_ST tiles) the sampling pass of knn_mfma_kernel visits with `splits` reference splits."""
    n_stages = (n_tiles + KNN_ST - 1) // KNN_ST
    sps = (n_stages + splits - 1) // splits
    out = set()
    for y in range(splits):
        s_begin, s_end = y * sps, min(n_stages, (y + 1) * sps)
        s_first = s_begin + min(y % sub, max(s_end - s_begin - 1, 0))
        out |= set(range(s_first, s_end, sub))
    return out


def decoy_units(n_tiles):
    """Stage sets of which EVERY sampling pass visits at least one, whatever split count (1 .. 16) the device picks and
    for the sampling steps 1 and 2: first the stages all of them visit, then disjoint pairs of adjacent stages."""
    n_stages = (n_tiles + KNN_ST - 1) // KNN_ST
    visits = [pass1_stages(n_tiles, sp) for sp in range(1, 17)]
    units, used = [], set()
    for s in range(n_stages):
        if all(s in v for v in visits):
            units.append((s,))
            used.add(s)
    s = 0
    while s + 1 < n_stages:
        if s not in used and s + 1 not in used and all(s in v or s + 1 in v for v in visits):
            units.append((s, s + 1))
            used |= {s, s + 1}
            s += 2
        else:
            s += 1
    return units


def _stage_rows(n1, n_tiles, stage):
    """Reference rows sitting in the tiles of `stage`: tile = row mod n_tiles in BOTH slot mappings of knn_slot_row."""
    r = np.arange(n1)
    return r[(r % n_tiles) // KNN_ST == stage]


def aligned_pair(seed, nq, n1, settle_k=TOP - 1, min_gap=10 * TIE_TOL * 1.02):
    """Queries and references on the bf16 grid +- 0.49 ulp(bf16) per channel (16 channels of magnitude ~2^-2, 16 of
    ~2^-3, random signs).  Query i = G_i + s_i d (d = 0.49 ulp, s_i random signs).  Its true neighbour t_i has the SAME
    residuals (aligned) on a grid point one ulp away from G_i in some channels; its decoy d_i sits on G_i with the
    OPPOSITE residuals.  The split drops lo.lo: d~ - D2 = +2 lo_q.lo_t for t_i and -2 lo_q.lo_d for d_i, so the decoy
    ranks first in the approximate distances although its float64 distance is larger by `gap` >= 10 TIE_TOL.
    The decoy (and, where no single stage is visited by every sampling pass, a near copy of it in the next stage) sits
    in tiles every sampling pass visits, the true neighbour in tiles of other stages.  Padding rows are random
    directions of slightly smaller norm.  meta: nn, decoy, copy [nq] rows (copy = decoy where there is none); gap [nq]
    float64, to the nearer of decoy and copy; frac [nq] = (err_t - err_d) / tau; inversion [nq] = (d~'(t) - d~'(decoy or
    copy, the larger)) / tau.  Queries are redrawn until tie-free at `settle_k`."""
    rng = np.random.default_rng(seed)
    n_tiles = (n1 + 31) // 32
    units = decoy_units(n_tiles)
    slots, used_stages = [], set()
    for un in units:                                  # one query per row of the unit's first stage
        rows = [_stage_rows(n1, n_tiles, s) for s in un]
        m = min(len(r) for r in rows)
        for j in range(m):
            slots.append(tuple(int(r[j]) for r in rows))
        used_stages |= set(un)
        if len(slots) >= nq:
            break
    if len(slots) < nq:
        raise ValueError(f'n1={n1}: room for {len(slots)} decoys only')
    slots = [slots[j] for j in rng.permutation(len(slots))[:nq]]
    r = np.arange(n1)
    spare = r[~np.isin((r % n_tiles) // KNN_ST, sorted(used_stages))]
    if len(spare) < nq:
        raise ValueError(f'n1={n1}: room for {len(spare)} true neighbours only')
    t_rows = rng.permutation(spare)[:nq]
    mag = np.where(np.arange(32) < 16, 0.25, 0.125)
    ulp = mag * 2.0 ** -7

    def triple():
        g = rng.permutation(32)                                       # which channels are the large ones
        m, u = mag[g], ulp[g]
        G = m * (1.0 + rng.integers(1, 5, 32) * 2.0 ** -7)            # mantissa 1 + j / 128, j in 1 .. 4
        sg = rng.choice([-1.0, 1.0], 32)                              # sign of the value
        s = rng.choice([-1.0, 1.0], 32)                               # sign of the residual
        q = (sg * G + s * 0.49 * u).astype(np.float32)
        d = (sg * G - s * 0.49 * u).astype(np.float32)
        d2 = d.copy()
        d2[0] = np.float32(sg[0] * G[0] - s[0] * 0.40 * u[0])         # the copy: one residual a little shorter
        gap_room = ((q.astype(np.float64) - d2.astype(np.float64)) ** 2).sum() - min_gap
        move = np.zeros(32)
        for c in rng.permutation(32):                                 # t: one ulp outwards while the gap holds
            if (move * u).dot(move * u) + u[c] ** 2 <= gap_room:
                move[c] = 1.0
        t = (sg * (G + move * u) + s * 0.49 * u).astype(np.float32)
        return q, t, d, d2

    na0 = float((mag * (1 + 2.5 / 128)) ** 2 @ np.ones(32))
    pad = rng.standard_normal((n1, 32))
    F1 = (pad / np.linalg.norm(pad, axis=1, keepdims=True) * np.sqrt(0.9 * na0)).astype(np.float32)
    F0 = np.zeros((nq, 32), np.float32)
    decoy = np.array([sl[0] for sl in slots])
    todo = np.ones(nq, bool)
    for _ in range(50):
        for i in np.nonzero(todo)[0]:
            q, t, d, d2 = triple()
            F0[i], F1[t_rows[i]], F1[slots[i][0]] = q, t, d
            if len(slots[i]) > 1:
                F1[slots[i][1]] = d2
        idx, D = f64_topk(F0, F1, settle_k + 1)
        todo = ~tie_free(idx, D, settle_k, None, 2 * TIE_TOL)
        if not todo.any():
            break
    else:
        raise RuntimeError('aligned queries did not settle')
    dp, na, nb, tau = emulate(F0, F1)
    i = np.arange(nq)
    Dt, Dd = d2_f64_of(F0, F1, t_rows[:, None])[:, 0], d2_f64_of(F0, F1, decoy[:, None])[:, 0]
    err_t, err_d = dp[i, t_rows] + na - Dt, dp[i, decoy] + na - Dd
    copy = np.array([sl[-1] for sl in slots])                       # the decoy itself where it has no copy
    Dc = d2_f64_of(F0, F1, copy[:, None])[:, 0]
    return Pair('aligned', F0, F1, nn=t_rows, decoy=decoy, copy=copy, slots=slots, gap=np.minimum(Dd, Dc) - Dt,
                frac=(err_t - err_d) / tau, inversion=(dp[i, t_rows] - np.maximum(dp[i, decoy], dp[i, copy])) / tau)


# ----------------------------------------------------------------------------------------------
# the batches
# ----------------------------------------------------------------------------------------------
BIG_N1 = (1024, 1100, 1537)
BIG_N0 = (45, 333, 777)
SMALL = {0: (61, 700), 12: (1, 1023), 25: (130, 5), 32: (97, 1023), 47: (50, 700), 63: (33, 5), 64: (75, 700)}
# call positions of the special pairs.  Every table (32 + 32 + 6) STARTS with a small pair and table 1 also ends with
# one, so the special pairs stand at 1, 31, 33 and 69 here and at 32, 63 and 64 (= 69 - 37, 69 - 6, 69 - 5) in the
# reversed order the route tests also run.
SPECIAL = {1: 'fallback_1e20', 5: 'fallback_nan', 6: 'dup33_b', 10: 'dup32', 15: 'wide64', 20: 'list64', 31: 'list65_a',
           33: 'dup33_a', 37: 'list65_b', 40: 'fallback_inf', 45: 'k_gt_n1', 50: 'aligned_b', 55: 'wide65', 69: 'aligned_a'}
N_PAIRS = 70
ALIGNED_NQ, ALIGNED_N1 = 90, 1100
BOUND_NQ, BOUND_N1 = 1500, 4704        # test d: 1500 queries in one pair


def _special(name, topk):
    base = name.rsplit('_', 1)[0] if name[-2:] in ('_a', '_b') else name
    seed = 1000 + sum(ord(ch) for ch in name)
    if name.startswith('fallback'):
        return fallback_pair(seed, {'1e20': 1e20, 'nan': np.nan, 'inf': np.inf}[name.split('_')[1]])
    if base == 'k_gt_n1':
        return random_pair('k_gt_n1', seed, 77, 20)
    if base == 'dup32':
        return cluster_pair('dup32', seed, 32, 40, 61)
    if base == 'dup33':
        return cluster_pair('dup33', seed, 33, 40, 61)
    if base in ('list64', 'list65'):
        n = 64 if base == 'list64' else 65
        if topk:   # the same boundary of the top-k search
            return cluster_pair('list256' if n == 64 else 'list257', seed, 2 * topk_slots(32) + 1, n + 192, 303 - n - 192,
                                n1=1537, start=200)
        return cluster_pair(base, seed, 33, n, 101 - n)
    if base in ('wide64', 'wide65'):
        n = int(base[4:])
        return cluster_pair(f'list{n}w', seed, 330, n, 101 - n)
    if base == 'aligned':
        return aligned_pair(seed, ALIGNED_NQ, ALIGNED_N1)
    raise KeyError(name)


_CACHE = {}


def batch(topk):
    """The 70 pairs of test a in call order; topk: list256 / list257 stand where list64 / list65 stand for 1-NN (every
    other pair is the same object in both batches)."""
    if topk in _CACHE:
        return _CACHE[topk]
    other = _CACHE.get(not topk)
    pairs = []
    for pos in range(N_PAIRS):
        name = SPECIAL.get(pos)
        if other is not None and not (name or '').startswith('list'):
            pairs.append(other[pos])
        elif pos in SMALL:
            pairs.append(random_pair('small', 100 + pos, *SMALL[pos]))
        elif name:
            pairs.append(_special(name, topk))
        else:
            pairs.append(random_pair('big', 100 + pos, BIG_N0[pos % 3], BIG_N1[(pos // 3) % 3]))
    _CACHE[topk] = pairs
    return pairs


def bound_pair():
    if 'bound' not in _CACHE:
        _CACHE['bound'] = aligned_pair(77, BOUND_NQ, BOUND_N1, settle_k=1)   # (a decoy and its copy tie at k = 2)
    return _CACHE['bound']


def orders():
    """Call orders of test a: as built, reversed, one seeded shuffle."""
    base = np.arange(N_PAIRS)
    return {'base': base, 'reversed': base[::-1].copy(), 'shuffled': np.random.default_rng(2024).permutation(N_PAIRS)}


def concat(pairs, order=None):
    """(F0, F1, off0, off1) of the pairs in `order`."""
    order = range(len(pairs)) if order is None else order
    ps = [pairs[int(j)] for j in order]
    off0 = np.concatenate([[0], np.cumsum([p.n0 for p in ps])]).astype(np.int64)
    off1 = np.concatenate([[0], np.cumsum([p.n1 for p in ps])]).astype(np.int64)
    return np.concatenate([p.F0 for p in ps]), np.concatenate([p.F1 for p in ps]), off0, off1


def width_batch(C, n_pairs=40, seed=5):
    """Test c: n_pairs pairs of width C (16 / 64: brute force throughout) with n1 in 5 .. 1500."""
    rng = np.random.default_rng(seed + C)
    n1 = np.concatenate([[5, 1500, 64, 65, 1023, 1024], rng.integers(5, 1501, n_pairs - 6)])
    n0 = np.concatenate([[1, 257, 1025], rng.integers(1, 400, n_pairs - 3)])
    return [Pair('width', unit(rng.standard_normal((int(a), C))), unit(rng.standard_normal((int(b), C))))
            for a, b in zip(n0, n1)]
