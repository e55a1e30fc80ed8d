"""Inputs of the kernel-map contract tests, each with the edge it is there for.

A case is tiny and states its edge as a precondition that `tests/test_maps_ref_cpu.py` asserts FROM THE ORACLE ALONE
(`Case.pre`): a case that stops reaching its edge fails there, on the CPU, not silently on the GPU.  The oracle of a
case is computed once per process and shared (`oracle_of`)."""
import numpy as np

import maps_ref as ref
from oracle import me_semantics as me


class Case:
    def __init__(self, name, D, make, why, ks=(3,), pre=None):
        self.name, self.D, self.make, self.why, self.ks, self._pre = name, D, make, why, tuple(ks), pre
        self._coords = None

    @property
    def coords(self):
        if self._coords is None:
            c = np.ascontiguousarray(self.make(), np.int32)
            assert c.ndim == 2 and c.shape[1] == self.D + 1
            assert len(np.unique(c, axis=0)) == len(c), 'duplicate rows in a case'
            self._coords = c
        return self._coords

    def pre(self, oracle):
        if self._pre:
            self._pre(self, oracle)

    def __repr__(self):
        return self.name


_ORACLES = {}


def oracle_of(case, ks=3):
    key = (case.D, case.name, ks)
    if key not in _ORACLES:
        _ORACLES[key] = ref.Oracle(case.coords, case.D, ks)
    return _ORACLES[key]


def with_batch(rows, b=0):
    rows = np.asarray(rows, np.int32)
    return np.concatenate([np.full((len(rows), 1), b, np.int32), rows], axis=1)


def cloud3(n, seed):
    """n distinct voxels of a box filled to about a third, centred on the origin (negative coordinates), in random order"""
    rng = np.random.default_rng(seed)
    s = max(2, int(np.ceil((3.0 * n) ** (1 / 3))))
    cells = rng.permutation(s ** 3)[:n]
    xyz = np.stack([cells % s, (cells // s) % s, cells // (s * s)], axis=1) - s // 2
    return with_batch(xyz)


def cloud6(n, seed):
    """n distinct 6-D rows shaped like the pipeline's: a voxel paired with a voxel near it, several rows per first half"""
    rng = np.random.default_rng(seed)
    base = cloud3(max(1, -(-n // 3)), seed + 1000)[:, 1:]
    first = base[rng.integers(0, len(base), 6 * n + 8)]
    rows = np.concatenate([first, first + 3 + rng.integers(-2, 3, first.shape)], axis=1)
    rows = rows[me.first_occurrence_unique(rows)][:n]
    assert len(rows) == n
    return with_batch(rows)


def lattice(shape, step=1, origin=0):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, len(shape))
    return g * step + origin


# ---------------------------------------------------------------------------------------------------------------
# preconditions (oracle only)
# ---------------------------------------------------------------------------------------------------------------
def pre_rows(n):
    def pre(case, o):
        assert len(case.coords) == n
        if n > 4096:
            # the rank of a coarse row that first occurs behind row 4096 needs the carry of the single-block scan
            keys = case.coords.copy()
            keys[:, 1:] = np.floor_divide(keys[:, 1:], 2) * 2
            first = me.first_occurrence_unique(keys)
            assert (first >= 4096).any() and (first < 4096).any()
        if n > 1 and case.D == 3:
            assert len(o.coords[2]) > 1 and len(o.coords[2]) < n
    return pre


def pre_line(n):
    def pre(case, o):
        k, _, _ = o.triplets('same', 1)
        per_rule = np.bincount(k, minlength=27)
        assert sorted(per_rule[per_rule > 0].tolist()) == [n - 1, n - 1, n], per_rule
        assert (per_rule == 0).sum() == 24          # most rules are empty
    return pre


def pre_lines_cover_tile_edges():
    """over the three lines: a rule with exactly 64 pairs, one with 65, one with 128"""
    sizes = set()
    for c in CASES_3D:
        if c.name.startswith('line'):
            sizes |= set(np.bincount(oracle_of(c).triplets('same', 1)[0], minlength=27).tolist())
    assert {63, 64, 65, 128, 129} <= sizes, sizes


def pre_lattice(case, o):
    k, _, out = o.triplets('same', 1)
    assert (np.bincount(k, minlength=27) > 0).all()
    assert np.bincount(out).max() == 27


def pre_isolated(case, o):
    for ks in case.ks:
        k, _, _ = oracle_of(case, ks).triplets('conv1', 1)
        assert (k == (ks ** 3) // 2).all() and len(k) == len(case.coords)
    for ts in ref.LEVELS:
        assert (o.triplets('same', ts)[0] == 13).all()


def pre_negative(case, o):
    assert case.coords[:, 1:].min() == -9 and case.coords[:, 1:].max() == 8
    for ts in (1, 2, 4):   # floor differs from truncation where a negative coordinate is no multiple of the new stride
        c = o.coords[ts][:, 1:]
        assert ((c < 0) & (c % (2 * ts) != 0)).any(), ts


def pre_mult8(case, o):
    assert (case.coords[:, 1:] % 8 == 0).all() and (case.coords[:, 1:] < 0).any()
    for ts in ref.LEVELS:
        assert len(o.coords[ts]) == len(case.coords)


def pre_two_batches(case, o):
    c = case.coords
    assert sorted(set(c[:, 0].tolist())) == [0, 5]
    a, b = c[c[:, 0] == 0][:, 1:], c[c[:, 0] == 5][:, 1:]
    assert np.array_equal(np.unique(a, axis=0), np.unique(b, axis=0))
    # every pair's input voxel also exists in the other batch (the cross-batch candidate), and no pair crosses
    for kind, ts in (('same', 1), ('same', 4), ('down', 2)):
        k, i, out = o.triplets(kind, ts)
        ts_in, ts_out = o.levels_of(kind, ts)
        bi, bo = o.coords[ts_in][i, 0], o.coords[ts_out][out, 0]
        assert len(k) and (bi == bo).all()
        other = o.coords[ts_in][i].copy()
        other[:, 0] = 5 - other[:, 0]
        assert (me.CoordIndex(o.coords[ts_in], 1).lookup(other) >= 0).all()


def pre_probe_wrap(case, o):
    c = case.coords
    assert len(c) == 64 and ref.table_capacity(64) == 128
    home = (ref.hash_rows(c) & np.uint64(127)).astype(np.int64)
    assert (home >= 126).sum() >= 6, home
    # absent queries (out + delta) that start inside the wrapped cluster: they must walk through it to an empty slot
    qh = _absent_query_slots(c)
    assert (qh >= 126).sum() >= 4 and (qh <= 1).sum() >= 4


def _absent_query_slots(c):
    """home slots (128-slot table) of the distinct 3^3 neighbour queries of the rows `c` that are not rows themselves"""
    q = np.repeat(c, 27, axis=0)
    q[:, 1:] += np.tile(me.kernel_offsets(3, 3), (len(c), 1)).astype(np.int32)
    q = np.unique(q[me.CoordIndex(c, 2).lookup(q) < 0], axis=0)
    return (ref.hash_rows(q) & np.uint64(127)).astype(np.int64)


def pre_replay(kind, ts, need_under=True, exact=False):
    def pre(case, o):
        lo, hi = ref.wave_records(o, kind, ts)
        region = ref.region_of(kind, ts)
        if exact:
            assert np.array_equal(lo, hi)
        assert (lo > region).any(), (int(lo.max()), region)          # a wave the placing pass must replay
        if need_under:
            assert (hi <= region).any()                              # and one it places from its records
        for kd, t in [('same', t) for t in ref.LEVELS] + [('down', t) for t in (1, 2, 4)]:
            assert len(o.triplets(kd, t)[0]) <= ref.CAP_ROW_6D * o.n_cap, (kd, t)
    return pre


def pre_sym_fine(case, o):
    assert len(case.coords) == 512 and len(o.triplets('same', 1)[0]) == 64000
    pre_replay('same', 1)(case, o)


def pre_hundreds(case, o):
    _, _, out = o.triplets('same', 1)
    per_row = np.bincount(out, minlength=o.n_cap)
    assert per_row.max() == 729 and (per_row > 255).sum() > 50


def pre_fits(case, o):
    assert len(o.triplets('same', 1)[0]) <= ref.CAP_ROW_6D * o.n_cap


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def _negative3():
    rng = np.random.default_rng(31)
    g = lattice((18, 18, 18), origin=-9)
    return with_batch(g[rng.permutation(len(g))[:1500]])


def _two_batches3():
    c = cloud3(300, 77)[:, 1:]
    rng = np.random.default_rng(78)
    both = np.concatenate([with_batch(c, 0), with_batch(c, 5)])
    return both[rng.permutation(len(both))]


def _probe_wrap():
    """64 rows of which eight hash to the last two slots of the 128-slot table; the other 56 are neighbours of those"""
    box = with_batch(lattice((13, 13, 13), origin=-6))
    home = (ref.hash_rows(box) & np.uint64(127)).astype(np.int64)
    last = box[home >= 126]
    offs = me.kernel_offsets(3, 3)
    for seed in range(400):      # the first draw whose absent neighbour queries also start at the table's last slots
        rng = np.random.default_rng(seed)
        heads = last[rng.permutation(len(last))[:8]]
        rows = [tuple(r) for r in heads.tolist()]
        while len(rows) < 64:
            h = heads[rng.integers(8)].copy()
            h[1:] += offs[rng.integers(27)].astype(np.int32)
            if tuple(h.tolist()) not in rows:
                rows.append(tuple(h.tolist()))
        rows = np.array(rows, np.int32)[rng.permutation(64)]
        qh = _absent_query_slots(rows)
        if (qh >= 126).sum() >= 4 and (qh <= 1).sum() >= 4:
            return rows
    raise AssertionError('no probe-wrap input found')


ROWS_3D_SMALL = (1, 63, 64, 65, 255, 256, 257, 513)
ROWS_3D_LARGE = (2047, 2048, 4096, 4097, 16384, 16385)

CASES_3D = (
    [Case(f'rows{n}', 3, (lambda n=n: cloud3(n, n)), 'wave / 256-row block / n_pad rounding edges', ks=(3, 5, 7), pre=pre_rows(n))
     for n in ROWS_3D_SMALL] +
    [Case(f'rows{n}', 3, (lambda n=n: cloud3(n, n)),
          'n_cap + 1 crosses SCAN_BLOCK (2047/2048); carry of scan_single_block (4096/4097); multi-block scan (16384/16385)',
          pre=pre_rows(n)) for n in ROWS_3D_LARGE] +
    [Case(f'line{n}', 3, (lambda n=n: with_batch(np.stack([np.arange(n) - 7, np.full(n, 2), np.full(n, -3)], 1))),
          'rules of exactly n and n - 1 pairs: the tile boundary', ks=(3, 5), pre=pre_line(n)) for n in (64, 65, 129)] +
    [Case('lattice6', 3, lambda: with_batch(lattice((6, 6, 6), origin=-2)), 'every offset present, interior rows have 27 pairs',
          ks=(3, 5, 7), pre=pre_lattice),
     Case('isolated', 3, lambda: with_batch(lattice((5, 5, 4), step=32, origin=-59)), 'only the centre rule is non-empty',
          ks=(3, 5, 7), pre=pre_isolated),
     Case('negative', 3, _negative3, 'coordinates in [-9, 8]: floor differs from truncation at every stride', ks=(3, 5), pre=pre_negative),
     Case('mult8', 3, lambda: with_batch(lattice((6, 5, 4), step=8, origin=-24)), 'all coordinates multiples of 8: no level shrinks',
          pre=pre_mult8),
     Case('two_batches', 3, _two_batches3, 'batches 0 and 5 with identical voxels: no pair may cross', ks=(3, 5), pre=pre_two_batches),
     Case('probe_wrap', 3, _probe_wrap, 'the probe chain of the 128-slot table wraps from mask to 0', pre=pre_probe_wrap)])


def _two_batches6():
    c = cloud6(400, 9)[:, 1:] - 11          # negative coordinates in both halves
    rng = np.random.default_rng(10)
    both = np.concatenate([with_batch(c, 0), with_batch(c, 5)])
    return both[rng.permutation(len(both))]


def _pre_two_batches6(case, o):
    assert (case.coords[:, 1:4] < 0).any() and (case.coords[:, 4:] < 0).any()
    pre_two_batches(case, o)
    pre_fits(case, o)


def _sym_fine(permute):
    g = lattice((4, 4, 4, 2, 2, 2))
    if permute:
        g = g[np.random.default_rng(12).permutation(len(g))]
    return with_batch(g)


def _strided():
    rng = np.random.default_rng(13)
    iso = lattice((10, 10, 10), step=16, origin=100)
    iso = np.concatenate([iso, iso[:, ::-1] + 3], axis=1)
    rows = np.concatenate([lattice((4, 4, 2, 4, 4, 4)), iso])
    # the lattice stays in front (its coarse rows share the first search waves), everything else in random order
    return with_batch(np.concatenate([rows[:2048][rng.permutation(2048)], rows[2048:][rng.permutation(1000)]]))


def _hundreds():
    """the input of test_gpu_maps.py::test_6d_maps_rows_with_hundreds_of_neighbours"""
    g = np.stack(np.meshgrid(*[np.arange(4)] * 6, indexing='ij'), -1).reshape(-1, 6)
    rng = np.random.default_rng(5)
    sparse = np.unique(rng.integers(20, 400, (24000, 6)), axis=0)
    rows = np.concatenate([g, sparse]).astype(np.int32)
    rows = rows[rng.permutation(len(rows))]
    return with_batch(rows)


def _lattice3x6():
    return with_batch(lattice((3,) * 6, origin=-1))


def _lattice3x6_fits():
    g = lattice((3,) * 6, origin=-1)
    return with_batch(g[np.random.default_rng(14).permutation(len(g))[:700]])


def _pre_overflow(case, o):
    assert len(case.coords) == 729 and len(o.triplets('same', 1)[0]) == 7 ** 6 > ref.CAP_ROW_6D * 729


CASES_6D = (
    [Case(f'rows{n}', 6, (lambda n=n: cloud6(n, n)), 'wave / 256-row block edges of the bit-matrix pipeline', pre=pre_fits)
     for n in (1, 64, 65, 256, 257)] +
    [Case('two_batches', 6, _two_batches6, 'two batches sharing every first half, negative coordinates in both halves',
          pre=_pre_two_batches6),
     Case('replay_sym_fine', 6, lambda: _sym_fine(False), 'same[0] waves beyond 256 records: symmetric replay, fine level',
          pre=pre_sym_fine),
     Case('replay_sym_fine_perm', 6, lambda: _sym_fine(True), 'the same under a row permutation', pre=pre_sym_fine),
     Case('replay_sym_ts8', 6, lambda: with_batch(lattice((4, 2, 2, 3, 3, 3), step=8, origin=-16)),
          'same[3] waves beyond 1024 records: symmetric replay on the dense renumbered level',
          pre=pre_replay('same', 8, need_under=False, exact=True)),
     Case('replay_strided', 6, _strided, 'down[0] waves beyond 256 records: strided replay with the in-major CSR',
          pre=pre_replay('down', 1, exact=True)),
     Case('hundreds', 6, _hundreds, 'rows with more than 255 pairs (16-bit rank prefixes)', pre=pre_hundreds)])

CASE_OVERFLOW = Case('lattice3x6', 6, _lattice3x6, '7^6 pairs > 160 * 729: capacity flag', pre=_pre_overflow)
CASE_FITS = Case('lattice3x6_fits', 6, _lattice3x6_fits, 'the same lattice with rows removed until it fits', pre=pre_fits)

ALL_CASES = CASES_3D + CASES_6D + [CASE_OVERFLOW, CASE_FITS]


def params(cases):
    """(case, ks, lean) of every run"""
    return [(c, ks, lean) for c in cases for ks in c.ks for lean in (False, True)]


def param_id(p):
    c, ks, lean = p
    return f'{c.D}d-{c.name}-ks{ks}-{"lean" if lean else "full"}'
