"""The kernel-map contract in numpy: what every array of a built maps object must hold.

Everything is derived from `oracle.me_semantics` (stride_coords, kernel_map, transposed_kernel_map): the reference is
the oracle's triplets in first-occurrence numbering.  The library numbers the rows of a renumbered level (6-D, ts >= 2)
in the order of their first-half buckets; that numbering is itself part of the contract (`expected_canon`), so every
array a conv kernel reads is determined exactly and is compared for equality -- integer work, no tolerance anywhere.

`Oracle` holds the reference of one input, `expected_*` state an array from it, `check_*` compare raw arrays (read back
with `ops.Maps.raw`) against them and raise AssertionError naming the array.  `read_all` fetches every array of one
object through a `read(kind, ts, field)` callable, `check_maps` runs the whole contract over them."""
import numpy as np

from oracle import me_semantics as me

LEVELS = (1, 2, 4, 8)
TILE_M = 64            # DGR_TILE_M: pairs per MFMA tile
OS_ROWS = 64           # DGR_OS_ROWS: the neighbour tables' row padding
CAP_ROW_6D = 160       # reserved pairs per row of a 6-D map (dgr_build_maps: cap_row)
# hit-list records a search wave may leave before the placing pass replays it (kmap.hip: KM_REGION = 512, km_region_of; the regions
# are KM_REGION / 2, and 2 * KM_REGION for the symmetric ts = 8 map).  The replay cases assert from these numbers that
# they reach the replay: if KM_REGION changes, their preconditions fail in test_maps_ref_cpu.py.
REGION_SYMMETRIC = 256        # KM_REGION / 2
REGION_SYMMETRIC_TS8 = 1024   # 2 * KM_REGION
REGION_STRIDED = 256          # KM_REGION / 2

_M32 = 0xffffffff


def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(_M32)


def hash_rows(rows):
    """dgr_hash_row (csrc/hash.h) restated on uint32 values held in uint64: [n, nc] int rows -> [n] hashes."""
    rows = np.asarray(rows).astype(np.int64)
    m = np.uint64(_M32)
    h = np.full(len(rows), 0x9747b28c, np.uint64)
    for d in range(rows.shape[1]):
        k = rows[:, d].astype(np.uint64) & m
        k = (k * np.uint64(0xcc9e2d51)) & m
        k = _rotl(k, 15)
        k = (k * np.uint64(0x1b873593)) & m
        h = h ^ k
        h = _rotl(h, 13)
        h = (h * np.uint64(5) + np.uint64(0xe6546b64)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & m
    h ^= h >> np.uint64(16)
    return h


def table_capacity(n_cap):
    """Slots of a coordinate hash over up to n_cap rows: the power of two >= max(2 n_cap, 64)."""
    cap = 64
    while cap < 2 * n_cap:
        cap *= 2
    return cap


def first_half_buckets(coords):
    """Bucket of every row of a 6-D level: buckets are the distinct first-half keys (b, x0, y0, z0), numbered in
    first-occurrence order."""
    _, first, inv = np.unique(np.asarray(coords)[:, :4], axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(first))
    return rank[np.asarray(inv).reshape(-1)]


def expected_canon(coords):
    """canon of a renumbered level: library row p holds the oracle's row canon[p].  Rows are grouped by first-half
    bucket, buckets in first-occurrence order, ascending oracle row inside a bucket."""
    return np.argsort(first_half_buckets(coords), kind='stable')


class Oracle:
    """The reference of one input: coordinates per level and kernel-map triplets, first-occurrence numbering."""

    def __init__(self, coords, D, conv1_ks=3):
        self.D, self.ks = D, conv1_ks
        self.coords = {1: np.asarray(coords, np.int32)}
        for ts in (2, 4, 8):
            self.coords[ts] = me.stride_coords(self.coords[ts // 2], ts)
        self.n_cap = len(self.coords[1])
        self._t = {}

    def renumbered(self, ts):
        return self.D == 6 and ts >= 2

    def canon(self, ts):
        """library row -> oracle row (identity on levels in the caller's order)"""
        key = ('canon', ts)
        if key not in self._t:
            n = len(self.coords[ts])
            self._t[key] = expected_canon(self.coords[ts]) if self.renumbered(ts) else np.arange(n)
        return self._t[key]

    def inv(self, ts):
        """oracle row -> library row"""
        c = self.canon(ts)
        out = np.empty(len(c), np.int64)
        out[c] = np.arange(len(c))
        return out

    def lib_coords(self, ts):
        return self.coords[ts][self.canon(ts)]

    def levels_of(self, kind, ts):
        """(ts of the input level, ts of the output level) of a map or table"""
        if kind in ('down', 'nbr_down'):
            return ts, 2 * ts
        if kind == 'nbr_up':
            return 2 * ts, ts
        return ts, ts

    def triplets(self, kind, ts):
        """(k, in, out) of the oracle, first-occurrence numbering, sorted by (k, out)"""
        key = (kind, ts)
        if key not in self._t:
            c, D = self.coords, self.D
            if kind in ('same', 'nbr_same'):
                t = me.kernel_map(c[ts], c[ts], D, 3, ts)
            elif kind == 'conv1':
                t = me.kernel_map(c[1], c[1], D, self.ks, 1)
            elif kind in ('down', 'nbr_down'):
                t = me.kernel_map(c[ts], c[2 * ts], D, 3, ts)
            elif kind == 'nbr_up':
                t = me.transposed_kernel_map(c[2 * ts], c[ts], D, 3, ts)
            else:
                raise KeyError(kind)
            self._t[key] = tuple(np.asarray(a, np.int64) for a in t)
        return self._t[key]

    def lib_triplets(self, kind, ts):
        """the same pairs in the library's numbering, sorted by (k, out): the rule-major order"""
        k, i, o = self.triplets(kind, ts)
        ts_in, ts_out = self.levels_of(kind, ts)
        i, o = self.inv(ts_in)[i], self.inv(ts_out)[o]
        order = np.lexsort((o, k))
        return k[order], i[order], o[order]


# ---------------------------------------------------------------------------------------------------------------
# expected arrays
# ---------------------------------------------------------------------------------------------------------------
def expected_rule_map(k, i, o, K, n_cap, strided):
    """Every array of a rule-major map from its pairs (k, in, out), library numbering, any order.  n_cap: the row
    capacity of the object (every level has the input's row count as its capacity)."""
    k, i, o = (np.asarray(a, np.int64) for a in (k, i, o))
    order = np.lexsort((o, k))
    k, i, o = k[order], i[order], o[order]
    P = len(k)
    per_rule = np.bincount(k, minlength=K)
    rule_ptr = np.concatenate([[0], np.cumsum(per_rule)])
    tiles = -(-per_rule // TILE_M)
    tile_ptr = np.concatenate([[0], np.cumsum(tiles)])
    T = int(tile_ptr[K])
    tk = np.repeat(np.arange(K), tiles)
    first = rule_ptr[tk] + TILE_M * (np.arange(T) - tile_ptr[tk])
    tile_desc = np.stack([tk, first, np.minimum(TILE_M, rule_ptr[tk + 1] - first), np.zeros(T, np.int64)], axis=1).reshape(-1, 4)
    e = dict(rule_ptr=rule_ptr, tile_ptr=tile_ptr, tile_desc=tile_desc, pair_in=i, pair_out=o, pair_k=k,
             # the output-major CSR: rows' pairs in ascending rule-major position, which is ascending k
             out_ptr=np.concatenate([[0], np.cumsum(np.bincount(o, minlength=n_cap))]),
             out_pos=np.argsort(o, kind='stable'), P=P)
    if strided:
        e['in_ptr'] = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n_cap))])
        e['in_pos'] = np.argsort(i, kind='stable')
    return e


def expected_nbr(k, i, o, n_cap):
    """Dense neighbour table [27, n_pad] from the pairs (k, in, out): -1 where there is no pair and on padding rows."""
    n_pad = -(-n_cap // OS_ROWS) * OS_ROWS
    t = np.full((27, n_pad), -1, np.int64)
    t[np.asarray(k), np.asarray(o)] = np.asarray(i)
    return t


def parity_classes(coords, ts):
    """Parity class of every row of a 3-D level: bit d = (coordinate d // ts) & 1, floor division."""
    c = np.asarray(coords).astype(np.int64)[:, 1:4]
    bits = np.floor_divide(c, ts) & 1
    return bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2)


# ---------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------
def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{name}: shape {got.shape}, expected {want.shape}'
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(bad[0])
        raise AssertionError(f'{name}: {len(bad)} of {got.size} entries differ, first at {at}: '
                             f'{got[at]} instead of {want[at]}')


def check_level(name, ocoords, coords, canon, renumbered):
    """coords / canon of one level against the oracle's coordinates (first-occurrence order)."""
    n = len(ocoords)
    assert len(coords) == n, f'{name}: {len(coords)} rows, expected {n}'
    if not renumbered:
        assert canon is None, f'{name}: a level in the caller\'s order has a canon'
        _same(f'{name}.coords', coords, ocoords)
        return
    assert canon is not None, f'{name}: a renumbered level without canon'
    assert len(canon) == n and np.array_equal(np.sort(canon), np.arange(n)), f'{name}.canon is not a permutation of range({n})'
    _same(f'{name}.coords vs oracle[canon]', coords, ocoords[canon])
    # grouped by first-half key, buckets in first-occurrence order, canon ascending inside a bucket
    b = first_half_buckets(ocoords)[canon]
    assert np.all(np.diff(b) >= 0), f'{name}: rows are not grouped by first-half bucket in first-occurrence order'
    assert np.all(np.diff(canon)[np.diff(b) == 0] > 0), f'{name}: canon is not ascending inside a bucket'
    _same(f'{name}.canon', canon, expected_canon(ocoords))


def probe_chains(coords, table, mask):
    """Length of every row's probe chain in a coordinate hash (slots visited from hash & mask up to the row's own
    slot), asserting the table's invariants on the way.  `coords` in the numbering the table's entries use."""
    table = np.asarray(table).astype(np.int64)
    n, cap = len(coords), len(table)
    assert cap == mask + 1 and cap & mask == 0, f'table of {cap} slots under mask {mask:#x}'
    filled = np.nonzero(table >= 0)[0]
    assert len(filled) == n, f'{len(filled)} non-empty slots for {n} rows'
    assert np.array_equal(np.sort(table[filled]), np.arange(n)), 'non-empty slots do not hold every row exactly once'
    slot_of = np.empty(n, np.int64)
    slot_of[table[filled]] = filled
    home = (hash_rows(coords) & np.uint64(mask)).astype(np.int64)
    dist = (slot_of - home) & mask
    # no empty slot in the cyclic range [home, home + dist]: the linear probe reaches the row before it gives up
    empties = np.concatenate([[0], np.cumsum(np.tile(table < 0, 2))])
    crossed = empties[home + dist + 1] - empties[home]
    assert not crossed.any(), f'{int((crossed > 0).sum())} rows sit behind an empty slot of their probe chain'
    return dist + 1, home, slot_of


def check_hash_table(name, coords, table, mask):
    try:
        return probe_chains(coords, table, mask)
    except AssertionError as e:
        raise AssertionError(f'{name}.table: {e}') from None


RULE_FIELDS = ('rule_ptr', 'tile_ptr', 'tile_desc', 'pair_in', 'pair_out', 'pair_k', 'out_ptr', 'out_pos', 'in_ptr', 'in_pos')


def rebuild_pair_out(out_ptr, out_pos, P):
    """pair_out of a lean map from its output-major CSR: what the row reduction of the forward relies on."""
    out_ptr, out_pos = np.asarray(out_ptr).astype(np.int64), np.asarray(out_pos).astype(np.int64)
    assert out_ptr[0] == 0 and np.all(np.diff(out_ptr) >= 0) and out_ptr[-1] == P, 'out_ptr is not a prefix sum ending at P'
    assert len(out_pos) == P and np.array_equal(np.sort(out_pos), np.arange(P)), 'out_pos is not a permutation of the pairs'
    pair_out = np.empty(P, np.int64)
    pair_out[out_pos] = np.repeat(np.arange(len(out_ptr) - 1), np.diff(out_ptr))
    return pair_out


def check_rule_map(name, raw, exp):
    """raw: dict field -> array (None: the build did not keep it) of one rule-major map; exp: expected_rule_map."""
    K = len(exp['rule_ptr']) - 1
    _same(f'{name}.rule_ptr', raw['rule_ptr'], exp['rule_ptr'])
    P = exp['P']
    assert int(raw['rule_ptr'][K]) == P
    pair_out = raw.get('pair_out')
    if pair_out is None:
        try:
            pair_out = rebuild_pair_out(raw['out_ptr'], raw['out_pos'], P)
        except AssertionError as e:
            raise AssertionError(f'{name}: {e}') from None
    pair_out = np.asarray(pair_out).astype(np.int64)
    assert len(pair_out) == P, f'{name}.pair_out: {len(pair_out)} entries, expected {P}'
    k = np.repeat(np.arange(K), np.diff(exp['rule_ptr']))
    assert np.all(np.diff(pair_out)[np.diff(k) == 0] > 0), f'{name}.pair_out is not strictly ascending inside every rule'
    _same(f'{name}.pair_out', pair_out, exp['pair_out'])
    _same(f'{name}.pair_in', raw['pair_in'], exp['pair_in'])
    if raw.get('pair_k') is not None:
        _same(f'{name}.pair_k', raw['pair_k'], exp['pair_k'])
    _same(f'{name}.out_ptr', raw['out_ptr'], exp['out_ptr'])
    _same(f'{name}.out_pos', raw['out_pos'], exp['out_pos'])
    if 'in_ptr' in exp:
        assert raw.get('in_ptr') is not None and raw.get('in_pos') is not None, f'{name}: a strided map without in-major CSR'
        _same(f'{name}.in_ptr', raw['in_ptr'], exp['in_ptr'])
        _same(f'{name}.in_pos', raw['in_pos'], exp['in_pos'])
    else:
        assert raw.get('in_ptr') is None and raw.get('in_pos') is None, f'{name}: a same-stride map with an in-major CSR'
    _same(f'{name}.tile_ptr', raw['tile_ptr'], exp['tile_ptr'])
    _same(f'{name}.tile_desc', raw['tile_desc'], exp['tile_desc'])


def check_nbr_table(name, nbr, n_pad, exp):
    assert n_pad == exp.shape[1], f'{name}.n_pad = {n_pad}, expected {exp.shape[1]}'
    _same(f'{name}.nbr', nbr, exp)


def check_classes(name, perm, cls_count, cls_cap, coords, ts, n_pad):
    """perm / cls_count of a transposed conv's table: the rows of every parity class, ascending (a stable counting
    sort: DgrNbrTable::perm)."""
    cls = parity_classes(coords, ts)
    perm, cls_count = np.asarray(perm), np.asarray(cls_count)
    assert cls_cap == n_pad and perm.shape == (8, cls_cap), f'{name}.perm: shape {perm.shape} under cls_cap {cls_cap}'
    _same(f'{name}.cls_count', cls_count, np.bincount(cls, minlength=8))
    assert int(cls_count.sum()) == len(coords), f'{name}.cls_count sums to {int(cls_count.sum())}, not {len(coords)}'
    for c in range(8):
        _same(f'{name}.perm[class {c}]', perm[c, :cls_count[c]], np.nonzero(cls == c)[0])


# ---------------------------------------------------------------------------------------------------------------
# the whole object
# ---------------------------------------------------------------------------------------------------------------
def _try(read, kind, ts, field):
    """The array, or None where the library refuses the field (ValueError: DGR_EINVAL)."""
    try:
        return read(kind, ts, field)
    except ValueError:
        return None


def present_maps(D, ks, lean):
    """The maps and tables a build makes: [(kind, ts)], and which optional fields each keeps."""
    out = []
    if D == 3:
        out += [('nbr_same', ts) for ts in LEVELS] + [('nbr_down', ts) for ts in (1, 2, 4)] + [('nbr_up', ts) for ts in (1, 2, 4)]
        if lean:
            return out
    out += [('same', ts) for ts in LEVELS] + [('conv1', 1)] + [('down', ts) for ts in (1, 2, 4)]
    return out


def kept_fields(D, kind, ts, lean):
    """(pair_out kept, pair_k kept, in-major CSR kept) of a rule-major map"""
    if kind == 'down':
        return True, not lean, True
    return not lean, (not lean) or ts == 1, False


def read_all(read, D, ks, lean):
    """Every field of every array the build made: {(kind, ts, field): array or int}.  Asserts on the way that exactly
    the fields the build should have kept exist, and that the others are refused."""
    got = {}
    for ts in LEVELS:
        for f in ('n', 'mask', 'coords', 'table'):
            got['level', ts, f] = read('level', ts, f)
        canon = _try(read, 'level', ts, 'canon')
        assert (canon is not None) == (D == 6 and ts >= 2), f'level {ts}: canon {"present" if canon is not None else "refused"}'
        if canon is not None:
            got['level', ts, 'canon'] = canon
    made = present_maps(D, ks, lean)
    for kind, ts in made:
        if kind.startswith('nbr'):
            for f in ('nbr', 'n_pad'):
                got[kind, ts, f] = read(kind, ts, f)
            perm = _try(read, kind, ts, 'perm')
            assert (perm is not None) == (kind == 'nbr_up'), f'{kind}[{ts}]: perm {"present" if perm is not None else "refused"}'
            if perm is not None:
                cc = read(kind, ts, 'cls_count')
                got[kind, ts, 'cls_count'], got[kind, ts, 'cls_cap'] = cc, read(kind, ts, 'cls_cap')
                # (entries behind a class's count are never written)
                got[kind, ts, 'perm'] = [perm[c, :max(0, min(int(cc[c]), perm.shape[1]))].copy() for c in range(8)]
                got[kind, ts, 'perm_shape'] = perm.shape
            continue
        want_out, want_k, want_in = kept_fields(D, kind, ts, lean)
        for f in ('rule_ptr', 'tile_ptr', 'tile_desc', 'pair_in', 'out_ptr', 'out_pos', 'pair_cap', 'n_cap', 'K'):
            got[kind, ts, f] = read(kind, ts, f)
        for f, want in (('pair_out', want_out), ('pair_k', want_k), ('in_ptr', want_in), ('in_pos', want_in)):
            a = _try(read, kind, ts, f)
            assert (a is not None) == want, f'{kind}[{ts}].{f}: {"present" if a is not None else "refused"}'
            if a is not None:
                got[kind, ts, f] = a
    # and what the build did not make is refused, not returned empty
    for kind, ts in (('same', 1), ('same', 8), ('conv1', 1), ('down', 4), ('nbr_same', 1), ('nbr_up', 4)):
        if (kind, ts) not in made:
            assert _try(read, kind, ts, 'nbr' if kind.startswith('nbr') else 'rule_ptr') is None, f'{kind}[{ts}] was not built but is readable'
    return got


def check_maps(got, oracle, lean, only=None):
    """The full contract over `read_all`'s result.  Returns per-level / per-map figures for the record.  `only`: the
    (kind, ts) to compare with the oracle (default: every map and table the build made; the levels always)."""
    D, ks, n_cap = oracle.D, oracle.ks, oracle.n_cap
    figures = {}
    for ts in LEVELS:
        oc = oracle.coords[ts]
        name = f'level[{ts}]'
        assert got['level', ts, 'n'] == len(oc), f'{name}: n = {got["level", ts, "n"]}, expected {len(oc)}'
        check_level(name, oc, got['level', ts, 'coords'], got.get(('level', ts, 'canon')), oracle.renumbered(ts))
        assert got['level', ts, 'mask'] == table_capacity(n_cap) - 1, f'{name}: mask {got["level", ts, "mask"]:#x}'
        chains, _, _ = check_hash_table(name, oracle.lib_coords(ts), got['level', ts, 'table'], got['level', ts, 'mask'])
        figures['level', ts] = dict(rows=len(oc), longest_probe_chain=int(chains.max()))
    for kind, ts in present_maps(D, ks, lean):
        if only is not None and (kind, ts) not in only:
            continue
        name = f'{kind}[{ts}]'
        k, i, o = oracle.lib_triplets(kind, ts)
        if kind.startswith('nbr'):
            check_nbr_table(name, got[kind, ts, 'nbr'], got[kind, ts, 'n_pad'], expected_nbr(k, i, o, n_cap))
            if kind == 'nbr_up':
                perm = np.full(got[kind, ts, 'perm_shape'], -1, np.int64)
                for c, rows in enumerate(got[kind, ts, 'perm']):
                    perm[c, :len(rows)] = rows
                check_classes(name, perm, got[kind, ts, 'cls_count'], got[kind, ts, 'cls_cap'], oracle.coords[ts], ts,
                              got[kind, ts, 'n_pad'])
            continue
        K = (ks if kind == 'conv1' else 3) ** D
        assert got[kind, ts, 'K'] == K and got[kind, ts, 'n_cap'] == n_cap, f'{name}: K {got[kind, ts, "K"]}, n_cap {got[kind, ts, "n_cap"]}'
        assert got[kind, ts, 'pair_cap'] == min(K, 1024 if D == 3 else CAP_ROW_6D) * n_cap, f'{name}: pair_cap {got[kind, ts, "pair_cap"]}'
        exp = expected_rule_map(k, i, o, K, n_cap, kind == 'down')
        check_rule_map(name, {f: got.get((kind, ts, f)) for f in RULE_FIELDS}, exp)
        per_row = np.diff(exp['out_ptr'])
        figures[kind, ts] = dict(pairs=exp['P'], largest_row=int(per_row.max()), largest_rule=int(np.diff(exp['rule_ptr']).max()),
                                 tiles=int(exp['tile_ptr'][K]))
    return figures


def assert_identical(a, b):
    """Two builds of the same input: every array `read_all` returns, bit for bit -- except the slot layout of the
    coordinate hash: which of two colliding rows claims the earlier slot depends on the order their threads ran in, and
    no consumer sees it (a look-up returns the same row either way; `check_hash_table` holds for both)."""
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    for key in a:
        if key[2] == 'table':
            _same(f'{key} rows (second build)', np.sort(b[key]), np.sort(a[key]))
        elif key[2] == 'perm':
            for c in range(8):
                _same(f'{key} class {c} (second build)', b[key][c], a[key][c])
        elif isinstance(a[key], np.ndarray):
            _same(f'{key} (second build)', b[key], a[key])
        else:
            assert a[key] == b[key], key


# ---------------------------------------------------------------------------------------------------------------
# search-wave model of the 6-D builder: hit records per wave of the search
# ---------------------------------------------------------------------------------------------------------------
def wave_records(oracle, kind, ts):
    """(lower, upper) bound of the hit records of every search wave of a 6-D map (kind 'same' | 'down').

    Search thread t = ja * n_cap + p handles first-half offset ja of the output row at position p of the output level's
    bucket order; a wave is 64 consecutive t.  Symmetric (same-stride) maps search ja = 0..13 and leave two records per
    hit -- the pair and its mirror -- except at the centre offset (one), and at ja = 13 only the offsets below the
    centre; strided maps search all 27 ja and leave one record per hit.  On a renumbered level position = library row,
    so the count is exact (lower == upper).  On level 0 the order inside a bucket is free: the bounds are the sums of
    the fewest / most records the wave's share of every bucket it covers can hold, valid for any such order."""
    assert oracle.D == 6 and kind in ('same', 'down')
    k, _, o = oracle.triplets(kind, ts)
    ts_out = oracle.levels_of(kind, ts)[1]
    n_out, n_cap = len(oracle.coords[ts_out]), oracle.n_cap
    ja, kb = k % 27, k // 27
    if kind == 'same':
        keep = (ja < 13) | ((ja == 13) & (kb <= 13))
        w = np.where(k == 364, 1, 2)[keep]
        ja, o, nj = ja[keep], o[keep], 14
    else:
        w, nj = np.ones(len(k), np.int64), 27
    rec = np.zeros((nj, n_out), np.int64)          # records of (ja, oracle output row)
    np.add.at(rec, (ja, o), w)
    n_waves = -(-nj * n_cap // 256) * 4            # whole 256-thread blocks of four waves
    lo, hi = np.zeros(n_waves, np.int64), np.zeros(n_waves, np.int64)
    if oracle.renumbered(ts_out):
        canon = oracle.canon(ts_out)
        for j in range(nj):
            np.add.at(lo, (j * n_cap + np.arange(n_out)) // 64, rec[j, canon])
        return lo, lo.copy()
    b = first_half_buckets(oracle.coords[ts_out])
    order = np.argsort(b, kind='stable')           # position -> row, up to the order inside a bucket
    pb = b[order]
    bucket_start = np.searchsorted(pb, pb)         # first position of the position's bucket
    for j in range(nj):
        r = rec[j, order]
        wave = (j * n_cap + np.arange(n_out)) // 64
        # segments: runs of positions in one bucket and one wave; a segment of c positions holds at least the c
        # smallest and at most the c largest record counts of its bucket
        new = np.concatenate([[True], (np.diff(pb) != 0) | (np.diff(wave) != 0)])
        seg = np.nonzero(new)[0]
        cnt = np.diff(np.concatenate([seg, [n_out]]))
        asc = np.concatenate([[0], np.cumsum(r[np.lexsort((r, pb))])])
        desc = np.concatenate([[0], np.cumsum(r[np.lexsort((-r, pb))])])
        sb = bucket_start[seg]
        np.add.at(lo, wave[seg], asc[sb + cnt] - asc[sb])
        np.add.at(hi, wave[seg], desc[sb + cnt] - desc[sb])
    return lo, hi


def region_of(kind, ts):
    if kind == 'down':
        return REGION_STRIDED
    return REGION_SYMMETRIC_TS8 if ts >= 8 else REGION_SYMMETRIC
