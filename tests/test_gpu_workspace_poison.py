"""Same bits whatever the workspace held: every public entry point must not depend on memory it was given but has not
written.

The library reserves worst-case capacities, bumps and rewinds one arena whose every stage starts on the previous one's
leftovers, and its tile kernels read past the valid extent on purpose; `ops` allocates its outputs with `torch.empty`.
The other suites check what a call computes from its inputs; this one checks what it must NOT compute from: for the
catalogue of tests/aux/poison_dump.py (every entry point at the smallest shapes with capacity slack and tile tails)

  1. workspace      results are the same bytes whatever the workspace and the library's private buffers held,
  2. neighbourhood  ... whatever lies next to the caller's inputs and in the caller's outputs before the call,
  3. extent         nothing is written outside the outputs.

The reference is the same call in an untouched process; there is no tolerance anywhere: every comparison is on bytes.

A ladder of child processes (one dump each, like tests/test_gpu_layer_trace.py), in this order:

  rung 0   DGR_WORKSPACE_FILL unset, twice: the two runs must agree on every key -- the catalogue's shapes fix every order
           of summation; a key that differs here is a finding of its own.
  rung 1   word 00000000   |  stale integers differ by one, stale floats by a denormal: a stale index or count that reaches
  rung 2   word 00000001   |  a result changes a value, while every address made from one stays small and valid.
  rung 3   word 7FC00000   every stale float is NaN (the NaN x 0 class); as an integer it is huge, so this rung runs only
           once rungs 1 and 2 matched rung 0 on every key.

The ladder stops at the first rung that differs or whose process ends abnormally and starts nothing after it.  With a
word set, the library fills its arena (every new chunk, every reset) and its other private allocations with it
(csrc/ctx.hip), the inputs lie between guard bands of it and `ops` allocates guarded outputs (tests/aux/poison.py); a
damaged band ends the child with a report.

The `peek` family is `dgr_debug_workspace_peek`: unwritten workspace words.  They are the word on rungs 1-3 (the fill
reaches the memory kernels get) and whatever the allocation held when unset, so for this one family "same bits" is
"same dtype and shape, every word the rung's".
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))

pytestmark = pytest.mark.gpu

FAMILIES = ('peek', 'voxelize', 'nets', 'maps', 'knn', 'glue', 'registration', 'o3d', 'fused', 'grids', 'posegraph',
            'voxelmean', 'tsdf')
RUNGS = (('rung0', None), ('rung0_again', None), ('rung1', '00000000'), ('rung2', '00000001'), ('rung3', '7FC00000'))
CHILD_TIMEOUT = 600


def family_of(key):
    return key.split('/', 1)[0]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(a, b, families=None):
    """Keys (of `families`) that the two dumps do not both hold with the same dtype, shape and bytes."""
    keys = sorted(set(a) | set(b))
    return [k for k in keys if (families is None or family_of(k) in families)
            and not (k in a and k in b and same_bytes(a[k], b[k]))]


class Ladder:
    def __init__(self):
        self.dumps, self.seconds, self.failed, self.stopped = {}, {}, None, None


@pytest.fixture(scope='module')
def ladder(tmp_path_factory):
    d = tmp_path_factory.mktemp('poison')
    L = Ladder()
    compared = [f for f in FAMILIES if f != 'peek']
    t_all = time.time()
    for name, word in RUNGS:
        env = {k: v for k, v in os.environ.items() if k != 'DGR_WORKSPACE_FILL'}
        if word is not None:
            env['DGR_WORKSPACE_FILL'] = word
        path = str(d / f'{name}.npz')
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'aux', 'poison_dump.py'), path], env=env,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            rc, tail = p.returncode, (p.stdout + p.stderr)[-3000:]
        except subprocess.TimeoutExpired as e:
            rc, tail = 'timeout', str(e)
        L.seconds[name] = time.time() - t0
        if rc != 0:
            L.failed = f'{name} (DGR_WORKSPACE_FILL={word}): the dump ended with {rc}\n{tail}'
            break
        with np.load(path) as z:
            L.dumps[name] = {k: z[k] for k in z.files}
        if name != 'rung0':
            diff = differing(L.dumps['rung0'], L.dumps[name], compared)
            if diff:
                L.stopped = f'{name} (DGR_WORKSPACE_FILL={word}) differs from rung 0 in {len(diff)} keys: {diff[:12]}'
                break
    L.seconds['module'] = time.time() - t_all
    keys = len(L.dumps.get('rung0', ()))
    print(f'poison ladder: {keys} keys per rung; seconds per rung '
          + ', '.join(f'{k} {v:.1f}' for k, v in L.seconds.items()))
    return L


def test_ladder_ran_to_rung_3_over_every_family(ladder):
    """Nothing skipped: no child failed (a damaged guard band ends one with its report), no rung stopped the ladder, every
    rung holds the same keys, and the keys cover every family of the catalogue."""
    assert ladder.failed is None, ladder.failed
    assert ladder.stopped is None, ladder.stopped
    assert list(ladder.dumps) == [name for name, _ in RUNGS]
    keys = set(ladder.dumps['rung0'])
    assert {family_of(k) for k in keys} == set(FAMILIES)
    for name, d in ladder.dumps.items():
        assert set(d) == keys, (name, sorted(set(d) ^ keys)[:12])


@pytest.mark.parametrize('family', FAMILIES)
def test_same_bits_at_every_rung(ladder, family):
    assert 'rung0' in ladder.dumps, ladder.failed
    base = ladder.dumps['rung0']
    mine = [k for k in base if family_of(k) == family]
    assert mine, f'no key of family {family}'
    for name, word in RUNGS[1:]:
        if name not in ladder.dumps:     # every rung that ran; a ladder that stopped early fails the ladder test
            continue
        d = ladder.dumps[name]
        if family == 'peek':
            for k in mine:
                assert k in d and d[k].dtype == base[k].dtype and d[k].shape == base[k].shape, (name, k)
                if word is not None:     # the fill is live
                    assert d[k].dtype == np.uint32 and (d[k] == np.uint32(int(word, 16))).all(), (name, k, d[k][:8])
            continue
        diff = differing(base, d, (family,))
        assert not diff, f'{name} (DGR_WORKSPACE_FILL={word}): {len(diff)} of {len(mine)} keys differ from rung 0: {diff[:12]}'
