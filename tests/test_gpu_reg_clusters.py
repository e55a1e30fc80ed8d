"""The registration kernel (csrc/reg.hip) at every cluster size, threshold and slice: non-chaotic comparisons with an f64
evaluation of the reference formulas (tests/reg_checks.py: the size grid, the weight patterns, the bounds and their
derivation; tests/test_reg_checks_cpu.py: the evidence that those bounds reject a dropped chunk, a member counted twice or
left out, a member total in f32 and a w > 0 compaction).  The measured tables are profiles/reg_procrustes_parity.txt and
profiles/reg_lossgrad_parity.txt (written when DGR_PARITY_REPORT names a directory)."""
import numpy as np
import pytest
import torch

import reg_checks as rc
from oracle import registration as oreg

pytestmark = pytest.mark.gpu
KW = dict(break_threshold_ratio=1e-4, quantization_size=rc.Q)


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def hip_procrustes(X, Y, w):
    from deepglobalregistration_amd import ops
    return ops.weighted_procrustes(*_dev(X, Y, w))


def hip_lossgrad(X, Y, w, prm, q):
    """Loss and gradient at `prm` out of ONE resumed step from zero moments: loss_prev = loss(prm), m = 0.1 grad,
    v = 0.001 grad^2 (reg.hip's Adam update) -- no trajectory, no sign-only first step."""
    from deepglobalregistration_amd import ops
    s0 = {'i': 0, 'prm': prm, 'm': np.zeros(9), 'v': np.zeros(9), 'loss_prev': 0.0, 'breaks': 0}
    out = ops.se3_refine_from(*_dev(X, Y, w), s0, 1, q, 10 ** 9, 1e-4)
    assert out['i'] == 1
    grad = out['m'] / float(np.float32(0.1))
    # v = 0.001f grad grad in f32: three roundings
    assert np.all(np.abs(out['v'] - float(np.float32(0.001)) * grad ** 2) <= 4 * rc.EPS32 * out['v'] + 1e-37), (out['v'], grad)
    return out['loss_prev'], grad


def _cases(n, patterns):
    for pattern in patterns:
        X, Y, out = rc.geometry(n)
        w = rc.weights(pattern, n, out)
        if w is not None:
            yield pattern, X, Y, w


def test_the_grid_covers_every_threshold_and_cluster_size():
    assert all(n in rc.GRID for n in (4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 6000, 12000, 30000))
    assert sorted({rc.cluster_size(n) for n in rc.GRID}) == [1, 2, 4, 8] and len(rc.GRID) == 22


@pytest.mark.parametrize('n', rc.GRID)
def test_weighted_procrustes_vs_f64(n):
    """Pass 1 (17 block sums; above 4095 rows the 17-value cluster exchange) over patterns (a) .. (f), on a cloud around the
    origin and on one 1e3 away from it (spread 1): R within bound_R, t within bound_t of the f64 evaluation -- the derived
    bounds alone wherever the rotation is well conditioned (gap >= 1e-3 s1), max(bound, 1.5 |f32 oracle - f64|) elsewhere.
    Derivation: tests/reg_checks.py.  Sizes / patterns with fewer than four surviving rows have no unique rotation: they
    are test_degenerate_inputs' business."""
    ran = 0
    for offset in (False, True):
        for pattern in rc.PATTERNS:
            X, Y, out = rc.geometry(n, offset)
            w = rc.weights(pattern, n, out)
            if w is None or np.count_nonzero(w) < 4:
                continue
            rc.check_procrustes(hip_procrustes, X, Y, w, f'hip {pattern}{"/offset" if offset else ""}')
            ran += 1
    assert ran or n < 4


@pytest.mark.parametrize('n', rc.GRID)
def test_loss_and_gradient_vs_f64(n):
    """The weighted loss and all nine gradient components of one iteration at a caller-chosen parameter vector (near: the
    Procrustes estimate turned by 1 degree and moved by 2 cm; far: most rows above the knee), patterns (a) .. (f), against
    autograd of the reference's loss in f64: per component |hip - f64| <= max(1.5 |f32 oracle - f64|, floor), the floor of
    tests/reg_checks.py (C_TERM = 8 roundings per term + the cancellation in p - y; at most 3 rows within 1e-5 of the knee).
    This is the check that sees a dropped chunk, overlapping compaction regions, a wrong member order or a mis-tagged
    exchange buffer: every row's term is in these sums exactly once."""
    for pattern, X, Y, w in _cases(n, rc.PATTERNS):
        for name, prm in rc.poses(X, Y, w).items():
            if rc.oracle_lossgrad(X, Y, w, prm, rc.Q, torch.float64)[0] < 1e-6:
                continue     # (signed weights on two rows: a negative loss, where the reference and the kernel stop before the gradient)
            rc.check_lossgrad(hip_lossgrad, X, Y, w, prm, tag=f'hip {pattern} {name}')


def _plane(n, seed, exact):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-2, 2, (n, 2))
    z = np.zeros(n) if exact else 0.3 * uv[:, 0] + 0.5 * uv[:, 1] + 0.7
    return np.column_stack([uv, z]).astype(np.float32)


@pytest.mark.parametrize('n', [3, 200, 4096, 16385])
@pytest.mark.parametrize('exact', [True, False])
@pytest.mark.parametrize('mirror', [False, True])
def test_coplanar_points_have_a_unique_rotation(n, exact, mirror):
    """Rank 2 exactly (z = 0: a zero column in the covariance, the completion branch of svd3.h) and up to rounding (a tilted
    plane): the rotation is unique and must match the f64 Kabsch of the oracle within the bounds of check_procrustes (gap =
    s2).  `mirror`: the target mirrored within the plane, which flips the sign of det(U) det(V) of the completed bases."""
    X = _plane(n, n, exact)
    Xs = X.astype(np.float64) * ([-1, 1, 1] if mirror else [1, 1, 1])
    Y = (Xs @ rc.ROT_GT.T + rc.T_GT).astype(np.float32)
    w = np.random.default_rng(n).uniform(0.5, 1, n).astype(np.float32)
    if mirror and not exact:
        # mirrored within its own plane: reflect across the plane through the origin spanned by (0, 1, 0.5) and the normal
        nrm = np.array([-0.3, -0.5, 1.0]); a = np.array([0.0, 1.0, 0.5]); m = np.cross(nrm, a); m /= np.linalg.norm(m)
        Xs = X.astype(np.float64) - [0, 0, 0.7]
        Xs = Xs - 2 * (Xs @ m)[:, None] * m
        Y = (Xs @ rc.ROT_GT.T + rc.T_GT).astype(np.float32)
    rc.check_procrustes(hip_procrustes, X, Y, w, f'hip coplanar exact={exact} mirror={mirror}', strict=True)


@pytest.mark.parametrize('n', [1, 2, 3, 300, 8192])
def test_degenerate_inputs(n):
    """Rank 1 and rank 0: collinear points (on an exact lattice line, where the covariance is rank 1 to f64 rounding and
    svd3.h completes two columns, and on a generic line) and one repeated point.  Asserted is what is well defined: R finite,
    orthonormal to f32 rounding, det R = 1, the line's direction mapped onto the target's, t = my - R mx."""
    rng = np.random.default_rng(n)
    k = rng.integers(-40, 40, (n, 1)).astype(np.float64)
    Rq = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])              # exact in f32
    lines = {'lattice': (k * np.array([1.0, 2.0, -1.0]) / 16, Rq, np.array([0.5, -0.25, 2.0])),
             'generic': (rng.uniform(-2, 2, (n, 1)) * np.array([0.3, -0.8, 0.52]) + [0.1, 0.2, 0.3], rc.ROT_GT, rc.T_GT),
             'point': (np.tile([[0.4, -1.3, 0.7]], (n, 1)), rc.ROT_GT, rc.T_GT)}
    for name, (Xd, Rg, tg) in lines.items():
        X = Xd.astype(np.float32)
        Y = (X.astype(np.float64) @ Rg.T + tg).astype(np.float32)
        w = rng.uniform(0.5, 1, n).astype(np.float32)
        R, t = hip_procrustes(X, Y, w)
        R, t = R.astype(np.float64), t.astype(np.float64)
        assert np.isfinite(R).all() and np.isfinite(t).all(), name
        assert abs(np.linalg.det(R) - 1) < 1e-5, (name, R)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 4 * rc.EPS32, (name, R)      # 3 products of f32-rounded entries
        w8 = w.astype(np.float64)[:, None] / (np.abs(w.astype(np.float64)).sum() + rc.EPS32)
        mx, my = (w8 * X).sum(0), (w8 * Y).sum(0)
        assert np.all(np.abs(t - (my - R @ mx)) <= 3 * rc.EPS32 * (np.abs(my) + np.abs(R) @ np.abs(mx))), (name, t)
        dx, dy = X.astype(np.float64) - mx, Y.astype(np.float64) - my
        if name != 'point' and np.abs(dx).max() > 1e-3:
            # every centred source point lies on the line and goes to its target: R d = d' (the sign included), to the f32
            # rounding of the inputs (|x|, |y| <= 8: 8 eps32 per coordinate, relative to a centred length >= 1e-3 ... 8)
            assert np.abs(dx @ R.T - dy).max() <= 64 * rc.EPS32, (name, np.abs(dx @ R.T - dy).max())


@pytest.mark.parametrize('n', [1000, 8192])
def test_all_weights_zero_is_the_identity(n):
    """Nothing to align: the covariance is exactly zero.  The kernel returns R = I, t = 0 and no error (svd3.h completes all
    three columns from the canonical axes); the oracle's LAPACK call returns a finite orthonormal R as well."""
    X, Y, _ = rc.geometry(n)
    R, t = hip_procrustes(X, Y, np.zeros(n, np.float32))
    assert np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
    Ro, to = oreg.weighted_procrustes(X, Y, np.zeros((n, 1), np.float32))
    assert torch.isfinite(Ro).all() and torch.isfinite(to).all() and (Ro.t() @ Ro - torch.eye(3)).abs().max() < 1e-6


@pytest.mark.parametrize('n,row', [(4096, 300), (8192, 3 * 256 + 17), (16385, 16383), (30000, 7 * 256 + 5)])
def test_non_finite_input_is_an_svd_error_through_the_exchange(n, row):
    """One NaN row in the chunks of a member other than member 0 (member 1 at 4096 rows, the last member elsewhere; at
    16385 rows the last row of member 7's last chunk, next to the one-row chunk 64 that goes back to member 0): the NaN has
    to travel through the 17-value exchange for every member to see it.  DGR_ESVD -> RuntimeError, not a pose."""
    from deepglobalregistration_amd import ops
    assert rc.member_of_row(n)[row] != 0
    X, Y, out = rc.geometry(n)
    w = rc.weights('a', n, out)
    w[row] = 0.8
    X[row, 1] = np.nan
    with pytest.raises(RuntimeError, match='SVD'):
        hip_procrustes(X, Y, w)
    with pytest.raises(RuntimeError, match='SVD'):
        ops.se3_refine(*_dev(X, Y, w), rc.Q, 50, 20, 1e-4)


@pytest.mark.parametrize('n', [4096, 8192, 12000, 16385])
def test_four_step_windows_at_clustered_sizes(n):
    """helpers.assert_window_accuracy (four steps from the f32 reference's own states vs four f64 steps) on one input per
    cluster size: the 13-value exchange over consecutive iterations, both `seq & 1` buffers."""
    from helpers import assert_window_accuracy
    X, Y, out = rc.geometry(n)
    assert_window_accuracy(X, Y, rc.weights('a', n, out), **KW)


@pytest.mark.parametrize('n', [4096, 8192, 16384])
def test_determinism_and_resume_bit_for_bit(n):
    """Two identical calls give identical bits; k steps + resume to K equals K steps in one launch (the resume test of
    test_gpu_knn_reg.py at clusters of 2, 4 and 8 -- every member takes the same Adam steps or this cannot hold)."""
    from deepglobalregistration_amd import ops
    X, Y, out = rc.geometry(n)
    Xg, Yg, wg = _dev(X, Y, rc.weights('a', n, out))
    a, b = (ops.se3_refine(Xg, Yg, wg, rc.Q, 1000, 20, 1e-4) for _ in range(2))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2]['iterations'] == b[2]['iterations'] and a[2]['break_count'] == b[2]['break_count']
    assert np.float32(a[2]['loss']).view(np.uint32) == np.float32(b[2]['loss']).view(np.uint32)
    R, t, st = ops.se3_refine(Xg, Yg, wg, rc.Q, 60, 10 ** 9, 1e-4)
    R0, t0 = ops.weighted_procrustes(Xg, Yg, wg)
    s0 = {'i': 0, 'prm': np.concatenate([R0[:, 0], R0[:, 1], t0]), 'm': np.zeros(9), 'v': np.zeros(9), 'loss_prev': 0.0, 'breaks': 0}
    mid = ops.se3_refine_from(Xg, Yg, wg, s0, 25, rc.Q, 10 ** 9, 1e-4)
    assert mid['i'] == 25
    end = ops.se3_refine_from(Xg, Yg, wg, mid, 60, rc.Q, 10 ** 9, 1e-4)
    one = ops.se3_refine_from(Xg, Yg, wg, s0, 60, rc.Q, 10 ** 9, 1e-4)
    assert np.array_equal(end['prm'], one['prm']) and np.array_equal(end['m'], one['m']) and np.array_equal(end['v'], one['v'])
    assert end['loss_prev'] == one['loss_prev'] and end['breaks'] == one['breaks']
    assert np.array_equal(one['prm'][6:].astype(np.float32), t.reshape(-1))


@pytest.mark.parametrize('n', [4096, 8192, 16384])
def test_stopping_decisions_through_the_exchange(n):
    """The two discrete outcomes that must agree with the oracle exactly (as test_refinement_golden holds them at cluster
    size 1): zero noise -> loss < 1e-7 at iteration 0 -> iterations == 0; an exhausted max_iter -> max_iter - 1."""
    from deepglobalregistration_amd import ops
    X, _, out = rc.geometry(n)
    Y = (X.astype(np.float64) @ rc.ROT_GT.T + rc.T_GT).astype(np.float32)
    w = np.random.default_rng(n).uniform(0.5, 1, n).astype(np.float32)
    R, t, st = ops.se3_refine(*_dev(X, Y, w), rc.Q, 1000, 20, 1e-4)
    Ro, to, so = oreg.global_registration(X, Y, w.reshape(-1, 1), **KW)
    assert so['iterations'] == 0 and st['iterations'] == 0 and st['break_count'] == so['break_count'] == 0
    # (the estimate itself is held to its bound by test_weighted_procrustes_vs_f64; here: it is returned untouched)
    assert np.abs(R - Ro).max() < 1e-6 and np.abs(t - to.reshape(-1)).max() < 1e-6
    X, Y, out = rc.geometry(n)
    w = rc.weights('a', n, out)
    R, t, st = ops.se3_refine(*_dev(X, Y, w), rc.Q, 7, 10 ** 9, 1e-4)
    so = oreg.global_registration(X, Y, w.reshape(-1, 1), max_iter=7, max_break_count=10 ** 9, **KW)[2]
    assert st['iterations'] == so['iterations'] == 6 and st['break_count'] == so['break_count']


# ---- the batch path through clusters and slices -------------------------------------------------------------------------
BATCH_ROWS = [16384] * 7 + [4096, 300, 8192, 16385, 5000, 1000]


def test_batch_through_every_cluster_size_and_a_second_launch():
    """One `register_batch` whose pair sizes force every cluster size in one launch, a slice boundary inside the batch and
    multi-member clusters at pair_base > 0.  A launch carries at most 64 members of multi-member clusters (reg.hip,
    REG_MAX_SPINNERS): 7 x 16384 rows = 7 x 8 = 56, 4096 rows + 2 = 58, 300 rows + 0 (a cluster of one does not spin),
    8192 rows + 4 = 62, 16385 rows + 8 = 70 > 64 -- so pairs 0 .. 9 are the first launch and pairs 10 (16385 rows, cluster
    of 8), 11 (5000 rows, cluster of 2) and 12 (1000 rows) the second one, with pair_base = 10.  149 661 rows per side.

    The nets run but do not influence the registration: every row has an override match and a forced logit.  Pair 12 is
    engineered to FAIL the gate just below it (200 rows at logit 6: wsum = 199.5 < max(200, 50)), pair 11 to pass just
    above it (252 rows: 251.4 >= max(200, 250)).  Every passing pair must be BIT-identical to `ops.se3_refine` called alone
    on its rows, its gathered matches and the batch's own weights: a pair's result depends on its row count only."""
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    voxel = 0.05
    ck = synth.synth_checkpoint(seed=0, voxel_size=voxel, feat_conv1_kernel_size=7)
    dgr = DeepGlobalRegistration({'weights': ck, 'clip_weight_thresh': 0.05}, torch.device('cuda'))
    clouds = []
    for s in (0, 1):
        a, b, T_gt = synth.synth_pair(s, n_raw=50000)
        (xa, ca, _), (xb, cb, _) = dgr.preprocess(a), dgr.preprocess(b)
        assert len(xa) >= 16385 and len(xb) >= 16385
        clouds.append((xa, ca, xb, cb, T_gt))
    rng = np.random.default_rng(3)
    x0, c0, x1, c1, off0, off1, ovr, logit = [], [], [], [], [0], [0], [], []
    for p, n in enumerate(BATCH_ROWS):
        xa, ca, xb, cb, T_gt = clouds[p % 2]
        xa, ca, xb, cb = xa[:n], ca[:n].clone(), xb[:n], cb[:n].clone()     # fragments of exact row counts
        ca[:, 0] = p; cb[:, 0] = p
        g = synth.gt_correspondences(xa.cpu().numpy(), xb.cpu().numpy(), T_gt, voxel, frac=1.0, seed=p)
        good = g >= 0
        idx = np.where(good, g, rng.integers(0, n, n))
        lg = np.where(good, rng.uniform(0, 4, n), rng.uniform(-6, -1.5, n))
        if n in (300, 5000, 1000):      # a fixed number of rows at logit 6, true matches first; everything else far below the clip
            k = {300: 250, 5000: 252, 1000: 200}[n]
            first = np.argsort(~good, kind='stable')[:k]
            lg = np.full(n, -6.0)
            lg[first] = 6.0
        x0.append(xa); c0.append(ca); x1.append(xb); c1.append(cb)
        ovr.append(idx + off1[-1]); logit.append(lg.astype(np.float32))
        off0.append(off0[-1] + n); off1.append(off1[-1] + n)
    assert off0[-1] == 149661
    C0, X0, C1, X1 = torch.cat(c0), torch.cat(x0), torch.cat(c1), torch.cat(x1)
    forced = np.concatenate(logit)
    # (a logit whose weight is within 1e-5 of the clip could fall on either side of it by the rounding of expf: moved away)
    forced[np.abs(1.0 / (1.0 + np.exp(-forced.astype(np.float64))) - 0.05) < 1e-5] = -6.0
    ovr = np.concatenate(ovr).astype(np.int64)
    T, status, stats = dgr.register_voxelized(C0, X0, off0, C1, X1, off1, override_idx1=torch.from_numpy(ovr).cuda(),
                                              forced_logits=torch.from_numpy(forced).cuda())
    assert np.array_equal(ops.batch_output('cuda', 'idx1').cpu().numpy(), ovr)
    wb = ops.batch_output('cuda', 'weights')
    w = wb.cpu().numpy()
    # weights: sigmoid in f64, clipped at 0.05; 1 / (1 + expf(-x)) is expf (2 ulp), an addition and a division: 4 eps32 of w <= 1
    w8 = 1.0 / (1.0 + np.exp(-forced.astype(np.float64)))
    assert not np.any(np.abs(w8 - 0.05) < 1e-6)                # no row sits on the clip itself
    w8[w8 < 0.05] = 0
    assert np.abs(w - w8).max() <= 4 * rc.EPS32 and np.array_equal(w == 0, w8 == 0)
    X0n, X1n = X0.cpu().numpy(), X1.cpu().numpy()
    expect_status = []
    for p, n in enumerate(BATCH_ROWS):
        s, e = off0[p], off0[p + 1]
        wsum = float(w[s:e].astype(np.float64).sum())
        assert abs(float(stats[p, 3]) - wsum) <= rc.EPS32 * wsum, (p, stats[p, 3], wsum)     # one f32 rounding of the f64 sum
        expect_status.append(0 if wsum >= max(200.0, 0.05 * n) else 1)
        if n == 5000:
            assert 250.0 <= wsum < 252.0
        if n == 1000:
            assert 199.0 < wsum < 200.0
    assert status.tolist() == expect_status and expect_status == [0] * 12 + [1]
    np.testing.assert_array_equal(T[12], np.eye(4))
    for p, n in enumerate(BATCH_ROWS[:12]):
        s, e = off0[p], off0[p + 1]
        Y = torch.from_numpy(X1n[ovr[s:e]]).cuda()
        R, t, st = ops.se3_refine(X0[s:e].contiguous(), Y, wb[s:e].contiguous(), 2 * voxel, 1000, 20, 1e-4)
        assert np.array_equal(T[p, :3, :3].astype(np.float32).view(np.uint32), R.view(np.uint32)), (p, n, T[p], R)
        assert np.array_equal(T[p, :3, 3].astype(np.float32).view(np.uint32), t.view(np.uint32)), (p, n, T[p], t)
        assert (int(stats[p, 0]), int(stats[p, 2])) == (st['iterations'], st['break_count']), (p, n, stats[p], st)
        assert np.float32(stats[p, 1]).view(np.uint32) == np.float32(st['loss']).view(np.uint32), (p, n, stats[p], st)
        print(f'batch pair {p:2d} n={n:6d} cluster {rc.cluster_size(n)} launch {1 if p < 10 else 2}: {st["iterations"]} iterations, '
              f'loss {st["loss"]:.4e}, bit-identical to the pair alone')
