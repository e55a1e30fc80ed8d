"""The registration checks of tests/reg_checks.py on the CPU, without a GPU: the f32 oracle and a CPU model of the kernel's
arithmetic (f32 per row, f64 sums per cluster member) are accepted at every grid size and weight pattern, and every broken
variant of the model is REJECTED at every clustered grid size where it differs from the model at all -- the evidence that
the bounds the GPU tests use are tight enough to see a dropped chunk, a member counted twice or not at all, a member total
rounded to f32, or a compaction that loses the negative weights.

Which check has to see which mutant:
  * drop_last_partial_chunk, member_twice, member_left_out: Procrustes AND loss/gradient, patterns (a) and (b); the first
    one only where n is not a multiple of 256 (elsewhere there is no partial chunk and the mutant is the model);
  * member_total_in_f32: Procrustes on the cloud 1e3 from the origin (the f32 rounding of a raw second moment of 1e6 is
    0.06, the covariance is ~0.1).  In the loss/gradient sums that rounding is below the per-term floor of a correct f32
    implementation by construction (eps32 / 2 of a partial sum <= eps32 C_TERM sum |terms|): not detectable there, and not
    claimed;
  * keep_w_gt_0: loss/gradient under pattern (f) (pass 1 does not go through the compaction)."""
import numpy as np
import pytest

import reg_checks as rc
from oracle import registration as oreg


def _oracle_procrustes(X, Y, w):
    R, t = oreg.weighted_procrustes(X, Y, w)
    return R.numpy(), t.numpy()


def _inputs(n, pattern, offset=False):
    X, Y, out = rc.geometry(n, offset)
    return X, Y, rc.weights(pattern, n, out)


def test_grid_is_the_issues_grid():
    assert set(rc.THRESHOLDS) <= set(rc.GRID) and {6000, 12000, 30000} <= set(rc.GRID) and len(rc.GRID) == 22
    assert [rc.cluster_size(n) for n in (4095, 4096, 8191, 8192, 16383, 16384)] == [1, 2, 2, 4, 4, 8]
    assert -(-12000 // rc.CHUNK) == 47 and 12000 % rc.CHUNK != 0
    own = rc.member_of_row(12000)
    assert [int((own == j).sum()) for j in range(4)] == [3072, 3072, 3040, 2816]     # 12, 12, 12 (the last one partial: 224 rows), 11 chunks


@pytest.mark.parametrize('n', rc.GRID)
def test_oracle_and_kernel_model_are_accepted(n, capsys):
    ran = 0
    for pattern in rc.PATTERNS:
        for offset in (False, True):
            X, Y, w = _inputs(n, pattern, offset)
            if w is None:
                continue
            tag = f'{pattern}{"/offset" if offset else ""}'
            if np.count_nonzero(w) >= 4:
                rc.check_procrustes(_oracle_procrustes, X, Y, w, tag + ' f32 oracle', strict=False)
                rc.check_procrustes(rc.model_procrustes, X, Y, w, tag + ' model')
                ran += 1
            if offset:
                continue
            for name, prm in rc.poses(X, Y, w).items():
                rc.check_lossgrad(rc.oracle_lossgrad, X, Y, w, prm, tag=f'{tag} {name} f32 oracle')
                rc.check_lossgrad(rc.model_lossgrad, X, Y, w, prm, tag=f'{tag} {name} model')
    assert ran or n < 4


def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('n', rc.CLUSTERED)
def test_every_mutant_is_rejected(n):
    seen = []
    for mutant in ('drop_last_partial_chunk', 'member_twice', 'member_left_out'):
        if rc.row_multiplier(mutant, n, np.ones(n)) is None:
            assert mutant == 'drop_last_partial_chunk' and n % rc.CHUNK == 0
            continue
        for pattern in ('a', 'b'):
            X, Y, w = _inputs(n, pattern)
            assert _rejected(rc.check_procrustes, lambda *a: rc.model_procrustes(*a, mutant=mutant), X, Y, w, mutant), (mutant, pattern)
            for name, prm in rc.poses(X, Y, w).items():
                assert _rejected(rc.check_lossgrad, lambda *a: rc.model_lossgrad(*a, mutant=mutant), X, Y, w, prm, tag=mutant), \
                    (mutant, pattern, name)
        seen.append(mutant)
    for pattern in ('a', 'b'):
        X, Y, w = _inputs(n, pattern, offset=True)
        assert _rejected(rc.check_procrustes, lambda *a: rc.model_procrustes(*a, mutant='member_total_in_f32'), X, Y, w, 'f32 total'), pattern
    X, Y, w = _inputs(n, 'f')
    assert (w < 0).sum() >= 10
    for name, prm in rc.poses(X, Y, w).items():
        assert _rejected(rc.check_lossgrad, lambda *a: rc.model_lossgrad(*a, mutant='keep_w_gt_0'), X, Y, w, prm, tag='w > 0'), name
    assert len(seen) == (2 if n % rc.CHUNK == 0 else 3)
