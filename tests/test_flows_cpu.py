"""The NumPy statement of the preserved-flow rule (tests/flows_cases.flow_rule, the reference of tests/test_gpu_flows.py) against the
oracle: applied to the oracle's full-list call of a sample it must give the oracle's own preserved call — the bases in preserved
order and the filter masks of every position that call parses.  No GPU."""
import numpy as np
import pytest

from oracle import pileup_oracle as po
from tests import flows_cases as fc


@pytest.fixture(scope="module")
def samples():
    return fc.oracle_samples()


def test_the_cases_are_what_they_say(samples):
    sm, full, preserved = samples
    assert len(sm) == 8 and full == sorted(full) and set(preserved) <= set(full) and len(set(preserved)) == len(preserved)
    assert preserved != sorted(preserved)                                  # shuffled
    no_line = [k for k in full if k[1] > 3000]
    assert len(no_line) == 5 and any(k in preserved for k in no_line)
    for data, excluded in sm:
        assert excluded <= set(full) and len(excluded) == len(full) * 3 // 10
        assert excluded & set(preserved) and excluded - set(preserved)     # excluded columns and excluded non-columns
    assert po.F_REGION == 32 == fc.F_REGION


@pytest.mark.parametrize("p", fc.ORACLE_PARAMS, ids=lambda p: "q%d-d%d-s%d-b%s" % (p.min_base_quality, p.min_cons_depth, p.min_cons_strand_depth,
                                                                                  p.min_cons_strand_bias))
def test_flow_rule_gives_the_oracles_preserved_call(samples, p):
    sm, full, preserved = samples
    rows = [fc.oracle_full_call(data, full, p) for data, _ in sm]
    base, filters, line_off = (np.stack([r[k] for r in rows]) for k in range(3))
    cols, col_of, excl_off, excl_slots = fc.flow_inputs(full, preserved, [e for _, e in sm])
    out_base, out_filters, err = fc.flow_rule(base, filters, line_off, cols, col_of, excl_off, excl_slots)
    assert err == 0
    compared = 0
    for s, (data, excluded) in enumerate(sm):
        compared += fc.check_against_oracle_preserved(data, full, preserved, excluded, p, out_base[s], out_filters[s])
    assert compared > 8 * len(preserved) // 2
    # the rule did something: Region set somewhere, a base turned into '-' somewhere, and it left alone what has no line
    assert ((out_filters & fc.F_REGION) != 0).any() and (out_base != base[:, cols]).any()
    assert not out_filters[line_off == 0].any()


def test_flow_rule_small_cases_by_hand():
    """The statement on the 3 x 37 case, spelled out entry by entry for sample 0's mixed list."""
    c = fc.small_case("subset", "mixed", bad_slots=True)
    ob, of, err = fc.flow_rule(c["base"], c["filters"], c["line_off"], c["cols"], c["col_of"], c["excl_off"], c["excl_slots"])
    assert err == 1
    lst = [int(x) for x in c["excl_slots"][c["excl_off"][0]:c["excl_off"][1]]]
    assert lst.count(37) == 1 and len(lst) == 9 and len(set(lst)) == 8
    a_col, not_col, _, no_line, first_line, malformed, has_region, twice, _ = lst
    assert c["col_of"][a_col] >= 0 and c["col_of"][not_col] < 0
    for slot in (a_col, not_col, first_line, has_region, twice):
        assert of[0, slot] == c["filters"][0, slot] | 32
        if c["col_of"][slot] >= 0:
            assert ob[0, c["col_of"][slot]] == 0x2D
    for slot in (no_line, malformed):
        assert of[0, slot] == c["filters"][0, slot]
        if c["col_of"][slot] >= 0:
            assert ob[0, c["col_of"][slot]] == c["base"][0, slot]
    assert np.array_equal(of[1], c["filters"][1]) and np.array_equal(ob[1], c["base"][1, c["cols"]])
    untouched = np.ones(37, dtype=bool)
    untouched[[s for s in lst if s < 37]] = False
    assert np.array_equal(of[0, untouched], c["filters"][0, untouched])
    for shape in ("empty", "identity"):
        c = fc.small_case(shape, "long")
        ob, of, err = fc.flow_rule(c["base"], c["filters"], c["line_off"], c["cols"], c["col_of"], c["excl_off"], c["excl_slots"])
        assert err == 0 and ob.shape == (3, len(c["cols"])) and list(np.diff(c["excl_off"])) == [257, 513, 1]
    c = fc.small_case("identity", "none")
    ob, of, err = fc.flow_rule(c["base"], c["filters"], c["line_off"], c["cols"], c["col_of"], c["excl_off"], None)
    assert err == 0 and np.array_equal(ob, c["base"]) and np.array_equal(of, c["filters"])
