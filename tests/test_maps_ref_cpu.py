"""The numpy contract of the kernel maps (tests/maps_ref.py) pinned on the CPU: hand-worked literals on tiny inputs, a
rejection for every kind of doctored array, and the precondition of every shared case (tests/maps_cases.py) asserted
from the oracle alone."""
import numpy as np
import pytest

import maps_cases as mc
import maps_ref as ref
from oracle import me_semantics as me


def line3():
    return ref.Oracle(np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0]], np.int32), 3, 3)


# the line of three voxels, by hand: rule 12 (dx = -1) pairs out 1 <- in 0, out 2 <- in 1; rule 13 the three centres;
# rule 14 (dx = +1) out 0 <- in 1, out 1 <- in 2
LINE3 = dict(
    rule_ptr=[0] * 13 + [2, 5] + [7] * 13,
    pair_in=[0, 1, 0, 1, 2, 1, 2], pair_out=[1, 2, 0, 1, 2, 0, 1], pair_k=[12, 12, 13, 13, 13, 14, 14],
    out_ptr=[0, 2, 5, 7], out_pos=[2, 5, 0, 3, 6, 1, 4],
    tile_ptr=[0] * 13 + [1, 2] + [3] * 13,
    tile_desc=[[12, 0, 2, 0], [13, 2, 3, 0], [14, 5, 2, 0]])


def line3_raw():
    return {f: (np.array(LINE3[f]) if f in LINE3 else None) for f in ref.RULE_FIELDS}


def test_line_of_three_by_hand():
    o = line3()
    exp = ref.expected_rule_map(*o.lib_triplets('same', 1), 27, 3, False)
    for f, want in LINE3.items():
        np.testing.assert_array_equal(exp[f], np.array(want), err_msg=f)
    ref.check_rule_map('line3', line3_raw(), exp)
    lean = line3_raw()
    lean['pair_out'] = lean['pair_k'] = None       # a lean map: pair_out rebuilt from the CSR
    ref.check_rule_map('line3 lean', lean, exp)
    np.testing.assert_array_equal(ref.expected_nbr(*o.lib_triplets('nbr_same', 1), 3)[12:15, :4],
                                  [[-1, 0, 1, -1], [0, 1, 2, -1], [1, 2, -1, -1]])


@pytest.mark.parametrize('lean', [False, True])
@pytest.mark.parametrize('doctor', ['out_pos_swap_in_row', 'tile_count', 'tile_first', 'pair_in', 'out_ptr', 'pair_k', 'rule_ptr'])
def test_rule_map_rejects_doctored_arrays(doctor, lean):
    o = line3()
    exp = ref.expected_rule_map(*o.lib_triplets('same', 1), 27, 3, False)
    raw = line3_raw()
    if lean:
        raw['pair_out'] = None
    if doctor == 'out_pos_swap_in_row':      # row 1 holds positions 0, 3, 6: the right pairs in the wrong order
        raw['out_pos'][[2, 3]] = raw['out_pos'][[3, 2]]
    elif doctor == 'tile_count':
        raw['tile_desc'][1, 2] = 64
    elif doctor == 'tile_first':
        raw['tile_desc'][2, 1] = 4
    elif doctor == 'pair_in':
        raw['pair_in'][[0, 1]] = raw['pair_in'][[1, 0]]
    elif doctor == 'out_ptr':
        raw['out_ptr'][1] = 3
    elif doctor == 'pair_k':
        raw['pair_k'][2] = 12
    elif doctor == 'rule_ptr':
        raw['rule_ptr'][14] = 4
    with pytest.raises(AssertionError):
        ref.check_rule_map('doctored', raw, exp)


def test_strided_map_and_its_in_major_csr():
    # four fine voxels on a line, two coarse ones: fine 0..3 -> coarse 0, 2; f = c + delta
    o = ref.Oracle(mc.with_batch(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])), 3, 3)
    k, i, out = o.lib_triplets('down', 1)
    # rule 12 (dx = -1): c=2 <- f=1; rule 13: c=0 <- f=0, c=2 <- f=2; rule 14: c=0 <- f=1, c=2 <- f=3
    assert (k.tolist(), i.tolist(), out.tolist()) == ([12, 13, 13, 14, 14], [1, 0, 2, 1, 3], [1, 0, 1, 0, 1])
    exp = ref.expected_rule_map(k, i, out, 27, 4, True)
    assert exp['in_ptr'].tolist() == [0, 1, 3, 4, 5] and exp['in_pos'].tolist() == [1, 0, 3, 2, 4]
    assert exp['out_ptr'].tolist() == [0, 2, 5, 5, 5] and exp['out_pos'].tolist() == [1, 3, 0, 2, 4]
    raw = {f: np.array(exp[f]) for f in ref.RULE_FIELDS}
    ref.check_rule_map('down', raw, exp)
    raw['in_pos'][[1, 2]] = raw['in_pos'][[2, 1]]      # fine row 1: rule 14 before rule 12
    with pytest.raises(AssertionError, match='in_pos'):
        ref.check_rule_map('down', raw, exp)
    # the transposed table pairs index and offset like the strided map it swaps
    kt, it, ot = o.lib_triplets('nbr_up', 1)
    assert (kt.tolist(), it.tolist(), ot.tolist()) == ([12, 13, 13, 14, 14], [1, 0, 1, 0, 1], [1, 0, 2, 1, 3])


def test_symmetric_map_without_its_mirrored_half_is_rejected():
    o = mc.oracle_of(mc.CASES_6D[1])          # 64 rows in 6-D
    k, i, out = o.lib_triplets('same', 1)
    assert (k > 364).any()
    exp = ref.expected_rule_map(k, i, out, 729, o.n_cap, False)
    half = k <= 364
    raw = ref.expected_rule_map(k[half], i[half], out[half], 729, o.n_cap, False)
    with pytest.raises(AssertionError):
        ref.check_rule_map('half', {f: raw.get(f) for f in ref.RULE_FIELDS}, exp)
    ref.check_rule_map('whole', {f: exp.get(f) for f in ref.RULE_FIELDS}, exp)


def test_parity_classes_of_a_block_with_negative_coordinates():
    block = mc.with_batch(mc.lattice((2, 2, 2), origin=-1))          # x slowest: (-1,-1,-1), (-1,-1,0), ...
    assert ref.parity_classes(block, 1).tolist() == [7, 3, 5, 1, 6, 2, 4, 0]
    b2 = block.copy()
    b2[:, 1:] *= 2
    assert ref.parity_classes(b2, 2).tolist() == [7, 3, 5, 1, 6, 2, 4, 0]
    assert ref.parity_classes(np.array([[0, -6, 4, -2]]), 2).tolist() == [0b101]     # -3 and -1 are odd
    rows = np.concatenate([block, block + [0, 2, 0, 0]])                               # 16 rows, two per class
    cls = ref.parity_classes(rows, 1)
    perm = np.full((8, 64), -1)
    for c in range(8):
        perm[c, :2] = np.nonzero(cls == c)[0]
    count = np.full(8, 2)
    ref.check_classes('t', perm, count, 64, rows, 1, 64)
    bad = perm.copy()
    bad[7, 0], bad[3, 0] = perm[3, 0], perm[7, 0]      # a row moved to the wrong class
    with pytest.raises(AssertionError):
        ref.check_classes('t', bad, count, 64, rows, 1, 64)
    bad = perm.copy()
    bad[5, :2] = perm[5, 1::-1]                         # the right rows, not ascending
    with pytest.raises(AssertionError):
        ref.check_classes('t', bad, count, 64, rows, 1, 64)
    with pytest.raises(AssertionError):
        ref.check_classes('t', perm, np.array([2, 2, 2, 2, 2, 2, 3, 1]), 64, rows, 1, 64)


def test_bucket_order_of_a_two_bucket_level():
    a, b = [0, 0, 0, 0], [0, 2, 0, 0]
    oc = np.array([a + [0, 0, 0], b + [0, 0, 0], a + [2, 0, 0], b + [2, 0, 0], a + [4, 0, 0]], np.int32)
    assert ref.first_half_buckets(oc).tolist() == [0, 1, 0, 1, 0]
    canon = ref.expected_canon(oc)
    assert canon.tolist() == [0, 2, 4, 1, 3]
    ref.check_level('l', oc, oc[canon], canon, True)
    for bad in ([0, 4, 2, 1, 3],            # not ascending inside the first bucket
                [1, 3, 0, 2, 4],            # buckets not in first-occurrence order
                [0, 2, 1, 4, 3],            # not grouped
                [0, 2, 4, 1, 1]):           # no permutation
        bad = np.array(bad)
        with pytest.raises(AssertionError):
            ref.check_level('l', oc, oc[bad], bad, True)
    with pytest.raises(AssertionError):
        ref.check_level('l', oc, oc[canon][::-1], canon, True)
    ref.check_level('l', oc, oc, None, False)
    with pytest.raises(AssertionError):
        ref.check_level('l', oc, oc[canon], None, False)


def insert_all(coords, cap):
    """A coordinate hash as the library's insertion leaves it when the rows arrive in row order."""
    table = np.full(cap, -1, np.int64)
    home = (ref.hash_rows(coords) & np.uint64(cap - 1)).astype(np.int64)
    for r, s in enumerate(home.tolist()):
        while table[s] >= 0:
            s = (s + 1) & (cap - 1)
        table[s] = r
    return table


def test_hash_of_known_rows():
    # dgr_hash_row over (0, 0, 0, 0) and (0, 1, -2, 3), worked through with Python integers
    def by_hand(row):
        m, h = 0xffffffff, 0x9747b28c
        rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & m   # noqa: E731
        for c in row:
            k = (c & m) * 0xcc9e2d51 & m
            k = rotl(k, 15) * 0x1b873593 & m
            h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & m
        h ^= h >> 16
        h = h * 0x85ebca6b & m
        h ^= h >> 13
        h = h * 0xc2b2ae35 & m
        return h ^ (h >> 16)
    rows = [[0, 0, 0, 0], [0, 1, -2, 3], [5, -9, 8, -1], [0, 1, 2, 3, 4, 5, 6]]
    for r in rows:
        assert int(ref.hash_rows(np.array([r]))[0]) == by_hand(r)


def test_hash_table_check():
    case = [c for c in mc.CASES_3D if c.name == 'probe_wrap'][0]
    coords = case.coords
    table = insert_all(coords, 128)
    chains, home, slot = ref.check_hash_table('t', coords, table, 127)
    assert (slot < home).any() and chains.max() >= 4          # the wrap: a row below its home slot
    # a row moved behind an empty slot is out of reach of the probe
    r = int(np.argmax(chains))
    bad = table.copy()
    bad[slot[r]] = -1
    free = [s for s in range(128) if bad[s] < 0 and bad[(s - 1) & 127] < 0 and s != slot[r]]
    bad[free[0]] = r
    with pytest.raises(AssertionError):
        ref.check_hash_table('t', coords, bad, 127)
    bad = table.copy()
    bad[slot[0]] = 1                                           # a row twice, another missing
    with pytest.raises(AssertionError):
        ref.check_hash_table('t', coords, bad, 127)
    bad = table.copy()
    bad[slot[0]] = -1                                          # a row missing
    with pytest.raises(AssertionError):
        ref.check_hash_table('t', coords, bad, 127)


def test_wave_model_by_hand():
    one = ref.Oracle(np.array([[0, 1, 2, 3, 4, 5, 6]], np.int32), 6, 3)
    lo, hi = ref.wave_records(one, 'same', 1)
    assert lo.tolist() == hi.tolist() == [1, 0, 0, 0]              # the centre pair: one record
    # two rows of one bucket, neighbours in the second half: two centre records, and the pair below the centre
    # (k = 13 + 27 * 12 = 337) with its mirror -- the pair above the centre is found from the other row
    two = ref.Oracle(np.array([[0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0]], np.int32), 6, 3)
    assert sorted(two.triplets('same', 1)[0].tolist()) == [337, 364, 364, 391]
    lo, hi = ref.wave_records(two, 'same', 1)
    assert lo.tolist() == hi.tolist() == [4, 0, 0, 0]
    # two rows in two buckets (first halves differ by one in x): ja = 12 finds row 0 from row 1: pair + mirror
    far = ref.Oracle(np.array([[0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0]], np.int32), 6, 3)
    lo, hi = ref.wave_records(far, 'same', 1)
    assert lo.tolist() == hi.tolist() == [4, 0, 0, 0]
    # strided: one record per hit, all 27 first-half offsets; coarse rows in bucket order (renumbered: exact)
    lo, hi = ref.wave_records(far, 'down', 1)
    assert np.array_equal(lo, hi) and lo.sum() == len(far.triplets('down', 1)[0]) == 2
    # level 0, a bucket split over two waves: the bounds take the fewest / most records of the bucket's rows
    g = mc.lattice((1, 1, 1, 5, 5, 4))                              # one bucket of 100 rows
    o = ref.Oracle(mc.with_batch(g), 6, 3)
    lo, hi = ref.wave_records(o, 'same', 1)
    k, _, out = o.triplets('same', 1)
    total = 2 * (k < 364).sum() + (k == 364).sum()
    assert lo.sum() <= total <= hi.sum() and (lo <= hi).all() and (lo < hi).any()


def model_read(o, lean):
    """A maps object as the contract states it, served through the `read` interface of maps_ref.read_all."""
    D, n_cap = o.D, o.n_cap
    made = ref.present_maps(D, o.ks, lean)

    def read(kind, ts, field):
        if kind == 'level':
            c = o.lib_coords(ts)
            if field == 'canon':
                if not o.renumbered(ts):
                    raise ValueError('no canon')
                return o.canon(ts)
            cap = ref.table_capacity(n_cap)
            return {'n': len(c), 'mask': cap - 1, 'coords': c, 'table': insert_all(c, cap)}[field]
        if (kind, ts) not in made:
            raise ValueError('not built')
        k, i, out = o.lib_triplets(kind, ts)
        if kind.startswith('nbr'):
            t = ref.expected_nbr(k, i, out, n_cap)
            if field in ('nbr', 'n_pad'):
                return t if field == 'nbr' else t.shape[1]
            if kind != 'nbr_up':
                raise ValueError('no classes')
            cls = ref.parity_classes(o.coords[ts], ts)
            if field == 'cls_count':
                return np.bincount(cls, minlength=8)
            if field == 'cls_cap':
                return t.shape[1]
            perm = np.full((8, t.shape[1]), 12345)
            for c in range(8):
                perm[c, :(cls == c).sum()] = np.nonzero(cls == c)[0]
            return perm
        K = (o.ks if kind == 'conv1' else 3) ** D
        e = ref.expected_rule_map(k, i, out, K, n_cap, kind == 'down')
        e.update(K=K, n_cap=n_cap, pair_cap=min(K, 1024 if D == 3 else ref.CAP_ROW_6D) * n_cap)
        keep_out, keep_k, _ = ref.kept_fields(D, kind, ts, lean)
        if field not in e or (field == 'pair_out' and not keep_out) or (field == 'pair_k' and not keep_k):
            raise ValueError('not kept')
        return e[field]
    return read


@pytest.mark.parametrize('D,name,ks', [(3, 'rows65', 5), (6, 'rows65', 3)])
@pytest.mark.parametrize('lean', [False, True])
def test_whole_contract_over_a_model_object(D, name, ks, lean):
    case = [c for c in (mc.CASES_3D if D == 3 else mc.CASES_6D) if c.name == name][0]
    o = mc.oracle_of(case, ks)
    got = ref.read_all(model_read(o, lean), D, ks, lean)
    fig = ref.check_maps(got, o, lean)
    assert fig['level', 1]['rows'] == 65
    ref.assert_identical(got, ref.read_all(model_read(o, lean), D, ks, lean))
    if not (D == 3 and lean):
        bad = dict(got)
        pos = got['down', 1, 'out_pos'].copy()
        row = int(np.argmax(np.diff(got['down', 1, 'out_ptr']) >= 2))
        s = int(got['down', 1, 'out_ptr'][row])
        pos[[s, s + 1]] = pos[[s + 1, s]]
        bad['down', 1, 'out_pos'] = pos
        with pytest.raises(AssertionError, match='out_pos'):
            ref.check_maps(bad, o, lean)
        with pytest.raises(AssertionError):
            ref.assert_identical(got, bad)


@pytest.mark.parametrize('case', mc.ALL_CASES, ids=lambda c: f'{c.D}d-{c.name}')
def test_case_reaches_its_edge(case):
    """the precondition of every shared case, from the oracle alone"""
    assert case.why
    case.pre(mc.oracle_of(case, case.ks[0]))


def test_lines_cover_the_tile_edges():
    mc.pre_lines_cover_tile_edges()


def test_region_constants_match_the_builder():
    """the replay preconditions rest on the hit-list region sizes: they are constants of the reference, tied to
    KM_REGION and the rule km_region_of of csrc/kmap.hip here so that a change of either fails loudly"""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, 'deepglobalregistration_amd', 'csrc', 'kmap.hip')).read()
    region = int(re.search(r'constexpr int KM_REGION = (\d+);', src).group(1))
    assert ('constexpr int km_region_of(int ts_in, bool symmetric) '
            '{ return (ts_in >= 8 && symmetric) ? 2 * KM_REGION : KM_REGION / 2; }') in src
    assert 'r.hl.region = km_region_of(J.in->ts, symmetric);' in src
    assert (ref.REGION_SYMMETRIC, ref.REGION_SYMMETRIC_TS8, ref.REGION_STRIDED) == (region // 2, 2 * region, region // 2)
