"""Every case of tests/fcgf_wide_cases.py reaches the edge it is there for: asserted from the oracle's maps alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fcgf_wide_cases as fc   # noqa: E402
import maps_ref as ref   # noqa: E402


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_case_reaches_its_edge(case):
    o = fc.oracle_of(case)
    case.pre(o)
    # ... and the contract's arrays of its three maps are well-formed statements of those pairs
    for kind, ts in fc.MAPS:
        k, i, out = o.lib_triplets(kind, ts)
        e = ref.expected_rule_map(k, i, out, 27, o.n_cap, False)
        assert e['P'] == len(k) and e['tile_ptr'][27] == len(e['tile_desc']) and 'in_ptr' not in e
        assert np.array_equal(ref.rebuild_pair_out(e['out_ptr'], e['out_pos'], e['P']), e['pair_out'])


def test_the_cases_cover_the_tile_edges_between_them():
    sizes = set()
    for case in fc.CASES:
        for kind, ts in fc.MAPS:
            sizes |= set(fc.per_rule(fc.oracle_of(case), kind, ts).tolist())
    assert 0 in sizes and 1 in sizes and any(0 < s < 64 for s in sizes) and any(64 < s < 128 for s in sizes) and any(s > 128 for s in sizes)
    assert set(fc.WIDE_LAYERS.values()) == set(fc.MAPS)
