"""The case builders of the batched k-NN route tests (tests/knn_cases.py) are what they claim to be -- proved from
float64 and an emulation of knn_pack_kernel's hi + lo bf16 split alone, without the library.

Measured for the committed seeds (printed by test_aligned_pairs_invert_the_ranking): over the `aligned` pairs the
approximation errors of true neighbour and decoy differ by 0.321 .. 0.381 of tau = KNN_TAU_C (na + max nb) (mean 0.348; a
naive construction with random mantissas reaches about 0.2), of which the float64 gap (2.07e-5 .. 2.37e-5, at least
10 TIE_TOL) takes its share: the decoy ranks 0.218 .. 0.282 tau BEFORE the true neighbour in the approximate distances.  A
bound of tau / 8 therefore loses the true neighbour of every such query; the committed bound keeps it."""
import numpy as np
import pytest

import knn_cases as kc

FRAC_MEASURED = 0.321      # smallest (err_t - err_d) / tau over the committed aligned pairs
INVERSION_MEASURED = 0.218 # smallest (d~'(t) - d~'(decoy)) / tau


@pytest.fixture(scope='module')
def batches():
    return {False: kc.batch(False), True: kc.batch(True)}


@pytest.fixture(scope='module')
def tops(batches):
    """float64 top-33 of every distinct pair, computed once."""
    out = {}
    for pairs in batches.values():
        for p in pairs:
            if id(p) not in out:
                out[id(p)] = kc.f64_topk(p.F0, p.F1)
    return out


def _aligned(batches):
    return [p for p in batches[False] if p.kind == 'aligned'] + [kc.bound_pair()]


def test_layout(batches):
    for topk, pairs in batches.items():
        assert len(pairs) == kc.N_PAIRS == 70
        kinds = [p.kind for p in pairs]
        for t0 in (0, 32, 64):
            assert kinds[t0] == 'small'                       # every table starts on the brute-force route
        assert kinds[63] == 'small'                           # table 1 also ends on it
        rev = kinds[::-1]
        special = {'fallback', 'dup33', 'aligned', 'list65', 'list257'}
        assert all(kinds[j] in special for j in (1, 31, 33, 69))
        assert all(rev[j] in special for j in (32, 63, 64))   # the reversed order puts special pairs on the table edges
        want = {'big', 'small', 'k_gt_n1', 'dup32', 'dup33', 'fallback', 'aligned'} | \
            ({'list256', 'list257'} if topk else {'list64', 'list65'}) | {'list64w', 'list65w'}
        assert set(kinds) == want
        assert sorted(p.meta['value'] != p.meta['value'] or p.meta['value'] for p in pairs if p.kind == 'fallback') \
            == [True, 1e20, np.inf]
        for p in pairs:
            assert p.F0.dtype == p.F1.dtype == np.float32 and p.F0.shape[1] == p.F1.shape[1] == 32
            if p.kind == 'big':
                assert p.n1 in (1024, 1100, 1537) and p.n0 % 32 != 0
            if p.kind == 'small':
                assert p.n1 in (5, 700, 1023)
            if p.kind == 'k_gt_n1':
                assert p.n1 == 20
            assert p.prefiltered == (p.kind not in ('small', 'k_gt_n1'))
        assert {p.n1 for p in pairs if p.kind == 'big'} == {1024, 1100, 1537}
        assert {p.n1 for p in pairs if p.kind == 'small'} == {5, 700, 1023}
        assert any(p.n0 == 1 for p in pairs if p.kind == 'small')
        # more than one x-block of the MFMA grid (16 query blocks) in some pair, and pairs of other sizes around it
        assert max(p.n0 for p in pairs) > 512
    same = [a is b for a, b in zip(batches[False], batches[True])]
    assert same.count(False) == 3                             # list64 / list65 (two of them) -> list256 / list257
    orders = kc.orders()
    assert all(sorted(o.tolist()) == list(range(70)) for o in orders.values())
    assert not np.array_equal(orders['shuffled'], orders['base']) and not np.array_equal(orders['shuffled'], orders['reversed'])


def test_no_ties_outside_the_clusters(batches, tops):
    """First / second and k-th / (k+1)-th float64 neighbours (in fact all of the first k + 1) more than TIE_TOL apart on
    EVERY query of the big, dup*, list* and aligned pairs, gaps inside a duplicate cluster excepted."""
    n = 0
    for pairs in batches.values():
        for p in pairs:
            if p.kind in ('small', 'k_gt_n1', 'fallback'):
                continue
            idx, D = tops[id(p)]
            for k in kc.KS:
                assert kc.tie_free(idx, D, k, p.cluster).all(), (p.kind, k)
            n += 1
    assert n >= 100
    p = kc.bound_pair()
    idx, D = kc.f64_topk(p.F0, p.F1, 2)     # the one-pair bound case: column 0 is what its test demands
    assert kc.tie_free(idx, D, 1).all()


def test_clusters_order_and_emulated_candidate_counts(batches, tops):
    """Beside a duplicate cluster the float64 neighbours are the cluster's rows in ascending order; the emulated
    candidates of such a query (d~' <= min d~' + tau) are the duplicates and nothing else: exactly 32 (dup32) and 33
    (dup33, list64, list65), 330 (list64w / list65w), 1025 > every slot count (list256 / list257).  The other queries of those pairs keep fewer
    than KNN_SLOTS references within tau of even their 16th approximate distance: they never overflow."""
    seen = set()
    for topk, pairs in batches.items():
        for p in pairs:
            if p.cluster is None or id(p) in seen:
                continue
            seen.add(id(p))
            lo, hi = p.cluster
            dup = hi - lo
            assert dup == {'dup32': 32, 'dup33': 33, 'list64': 33, 'list65': 33, 'list64w': 330, 'list65w': 330, 'list256': 1025,
                           'list257': 1025}[p.kind]
            assert len(p.near) == {'dup32': 40, 'dup33': 40, 'list64': 64, 'list65': 65, 'list64w': 64, 'list65w': 65,
                                   'list256': 256, 'list257': 257}[p.kind]
            assert np.all(p.F1[lo:hi] == p.F1[lo])
            assert np.linalg.norm(p.F0[p.near].astype(np.float64) - p.F1[lo].astype(np.float64), axis=1).max() < 1e-4
            c = p.F1[lo].astype(np.float64)
            rest = np.r_[0:lo, hi:p.n1]
            assert (p.F1[rest].astype(np.float64) @ c).max() < -0.39           # the opposite half-space, deep
            idx, D = tops[id(p)]
            m = min(kc.TOP, dup)
            np.testing.assert_array_equal(idx[p.near, :m], np.tile(np.arange(lo, lo + m), (len(p.near), 1)))
            dp, na, nb, tau = kc.emulate(p.F0, p.F1)
            cand = dp <= dp.min(1, keepdims=True) + tau[:, None]
            assert np.all(cand[p.near].sum(1) == dup)
            assert np.all(cand[p.near][:, lo:hi])
            far = np.setdiff1d(np.arange(p.n0), p.near)
            d16 = np.sort(dp[far], axis=1)[:, 15:16]
            assert ((dp[far] <= d16 + tau[far, None]).sum(1) < kc.KNN_SLOTS).all()
            assert not cand[far][:, lo:hi].any()
            if p.kind.startswith('list25'):
                assert dup == 2 * kc.topk_slots(32) + 1 and all(dup > kc.topk_slots(k) for k in (2, 8, 32))
    assert len(seen) == 11


def test_aligned_pairs_invert_the_ranking(batches):
    fr, inv, gaps = [], [], []
    for p in _aligned(batches):
        m = p.meta
        idx, D = kc.f64_topk(p.F0, p.F1, 3)
        np.testing.assert_array_equal(idx[:, 0], m['nn'])                  # float64: the aligned row is the neighbour
        i = np.arange(p.n0)
        second = np.where(m['copy'] != m['decoy'], m['copy'], m['decoy'])  # the copy is a little nearer than the decoy
        np.testing.assert_array_equal(idx[:, 1], second)
        gap = D[:, 1] - D[:, 0]
        assert gap.min() >= 10 * kc.TIE_TOL                                # ... and not by a tie
        np.testing.assert_allclose(gap, m['gap'], rtol=1e-9)
        dp, na, nb, tau = kc.emulate(p.F0, p.F1)
        worst = np.maximum(dp[i, m['decoy']], dp[i, m['copy']])            # whichever of the two a sampling pass sees
        assert np.all(worst < dp[i, m['nn']])                              # emulated: the decoy ranks first
        assert np.all(np.isin(dp.argmin(1), np.stack([m['decoy'], m['copy']])) &
                      ((dp.argmin(1) == m['decoy']) | (dp.argmin(1) == m['copy'])))   # ... of all references
        err_t = dp[i, m['nn']] + na - D[:, 0]
        Dd = kc.d2_f64_of(p.F0, p.F1, m['decoy'][:, None])[:, 0]
        err_d = dp[i, m['decoy']] + na - Dd
        assert np.all(np.abs(err_t) < tau / 2) and np.all(np.abs(err_d) < tau / 2)   # what the bound promises
        assert np.all(Dd - D[:, 0] < np.abs(err_t) + np.abs(err_d))
        frac, inversion = (err_t - err_d) / tau, (dp[i, m['nn']] - worst) / tau
        np.testing.assert_allclose(frac, m['frac'], rtol=1e-9)
        fr.append(frac), inv.append(inversion), gaps.append(gap)
        # grid +- 0.49 ulp(bf16): the split leaves hi on the grid and |lo| = 0.49 ulp
        hi, lo = kc.split(p.F0)
        ulp = 2.0 ** (np.floor(np.log2(np.abs(hi))) - 7)
        np.testing.assert_allclose(np.abs(lo) / ulp, 0.49, atol=2e-3)
        # the decoy (or its copy) sits in tiles every sampling pass visits, the true neighbour in other stages; the tile
        # of a row is row mod n_tiles in both slot mappings of knn_slot_row
        n_tiles = (p.n1 + 31) // 32
        for topk in (False, True):
            s, t = np.meshgrid(np.arange(32), np.arange(n_tiles), indexing='ij')
            row = (((s + t) & 31) if topk else s) * n_tiles + t
            assert np.all(row % n_tiles == t) and len(np.unique(row)) == row.size
        stage = lambda r: (np.asarray(r) % n_tiles) // kc.KNN_ST   # noqa: E731
        for sp in range(1, 17):
            seen = np.array(sorted(kc.pass1_stages(n_tiles, sp, 2)))
            hit = np.array([np.isin(stage(list(sl)), seen).any() for sl in m['slots']])
            assert hit.all(), sp
            assert kc.pass1_stages(n_tiles, sp, 1) == set(range((n_tiles + kc.KNN_ST - 1) // kc.KNN_ST))
        used = {int(s) for sl in m['slots'] for s in stage(list(sl))}
        assert not (set(stage(m['nn']).tolist()) & used)
    fr, inv, gaps = np.concatenate(fr), np.concatenate(inv), np.concatenate(gaps)
    print(f'aligned: (err_t - err_d) / tau = {fr.min():.3f} .. {fr.max():.3f} (mean {fr.mean():.3f}); decoy ahead by '
          f'{inv.min():.3f} .. {inv.max():.3f} tau; float64 gap {gaps.min():.3g} .. {gaps.max():.3g}')
    assert fr.min() >= 0.9 * FRAC_MEASURED
    assert inv.min() >= 0.9 * INVERSION_MEASURED > 1 / 8      # tau / 8 drops the true neighbour, tau keeps it
    assert inv.max() < 1


def test_f32_kernel_distances_are_within_the_tolerance(batches, tops):
    """The operation order of knn_d2, emulated: on these shapes the f32 distances of the float64 neighbours are within the
    1e-6 the GPU module demands, squared or not, so a failure there is the kernel's."""
    worst = 0.0
    for p in batches[True] + [q for q in batches[False] if q.kind.startswith('list')]:
        idx, D = tops[id(p)]
        d2 = kc.d2_f32_kernel(p.F0, p.F1, idx).astype(np.float64)
        ok = np.isfinite(D)
        np.testing.assert_allclose(d2[ok], D[ok], atol=1e-6)
        np.testing.assert_allclose(np.sqrt(d2[ok].astype(np.float32) + np.float32(1e-7)), np.sqrt(D[ok] + 1e-7), atol=1e-6)
        worst = max(worst, np.abs(d2[ok] - D[ok]).max())
    print(f'emulated f32 knn_d2 against float64: worst {worst:.3g}')


def test_width_batches():
    for C in (16, 64):
        ps = kc.width_batch(C)
        assert len(ps) == 40 and all(p.F0.shape[1] == C for p in ps)
        assert min(p.n1 for p in ps) == 5 and max(p.n1 for p in ps) == 1500
