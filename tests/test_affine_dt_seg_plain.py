"""The plain segmented traceback of tests/affine_dt_seg_plain.py against the plain ends-free diagonal transition of
tests/affine_dt_ends_plain.py: cost, start, end and CIGAR string are equal, over the pairs of tests/affine_dt_seg_cases.py and the DT lists
that bear on the walk, globally under all seven models and in every ends-free setting under SETTING_MODELS, at five segment lengths
(E, E + 1, 2E - 1, the default, one above every cost) and three bounds (none, the list's largest cost, that minus one).  The store of the
restatement raises on a read outside the segment's E head rows and the segment, so every run is also a test of the E-rows argument.
The last test asserts that the runs stood at the edges they are meant to cover."""
import pytest

from tests import affine_dt_cases as dt_cases
from tests import affine_dt_ends_cases as ends_cases
from tests import affine_dt_seg_cases as cases
from tests.affine_dt_ends_plain import affine_dt_ends
from tests.affine_dt_seg_plain import _Window, affine_dt_seg, bound_of, max_edge, seg_of

MODELS = cases.MODELS
BIG = (1 << 30) - 1
NOT_FOUND = (-1, -1, -1, "")
LISTS = dict(cases.all_cases(), tails=dt_cases.tails(), low_complexity=dt_cases.low_complexity(), far_diagonals=dt_cases.far_diagonals(),
             tied=ends_cases.tied(), lengths=dt_cases.lengths()[::7])
PARAMS = [(name, (False, False)) for name in sorted(MODELS)] + [(name, s) for name in ends_cases.SETTING_MODELS for s in ends_cases.SETTINGS if s != (False, False)]
_ORACLE = {}
SEEN = []  # (cost, seg, nseg, crossed) of every found run, for the last test


def oracle(a, b, name, fs, fe):
    key = (a, b, name, fs, fe)
    if key not in _ORACLE:
        _ORACLE[key] = affine_dt_ends(a, b, MODELS[name], BIG, fs, fe)
    return _ORACLE[key]


def segs_of(E, top):
    return (E, E + 1, max(2 * E - 1, E), 0, top + E + 1)


def run_list(pairs, name, fs, fe, segs=None):
    """Every pair at every seg without a bound.  Under a bound the restatement computes, for a found pair at an explicit seg, exactly
    what it computes without one (the bound enters through the default seg and through not finding a pair), so the bounded runs are
    the default seg for every pair, and every seg for the pairs the bound cuts off."""
    cm = MODELS[name]
    E = max_edge(cm)
    want = [oracle(a, b, name, fs, fe) for a, b in pairs]
    top = max(w[0] for w in want)
    for s_max in (BIG, top, max(top - 1, 0)):
        for seg in segs or segs_of(E, top):
            for (a, b), w in zip(pairs, want):
                if s_max != BIG and seg != 0 and w[0] <= s_max:
                    continue
                got = affine_dt_seg(a, b, cm, s_max, seg, fs, fe)
                assert got[:4] == (w if w[0] <= s_max else NOT_FOUND), (len(a), len(b), s_max, seg)
                rec = got[4]
                assert rec["seg"] == seg_of(bound_of(len(a), len(b), cm, s_max, fs, fe), E, seg)
                if got[0] >= 0:
                    assert rec["nseg"] == got[0] // rec["seg"] + 1 and len(rec["crossed"]) == rec["nseg"] - 1
                    SEEN.append((got[0], rec["seg"], rec["nseg"], tuple(rec["crossed"])))
                else:
                    assert rec["nseg"] == 0 and rec["crossed"] == []


@pytest.mark.parametrize("name,setting", PARAMS, ids=["%s-fs%d-fe%d" % (n, *s) for n, s in PARAMS])
@pytest.mark.parametrize("case", sorted(LISTS))
def test_results_equal_the_unsegmented_walk(case, name, setting):
    # (the 2 kbp pair is there for its many segments: the default seg and the shortest one)
    run_list(LISTS[case], name, *setting, segs=(max_edge(MODELS[name]), 0) if case == "many" else None)


def test_the_store_raises_outside_the_head_and_the_segment():
    F = _Window()
    F.put(5, 0, ([1], [2], [3]))
    assert F.at(0, 5, 0) == 1 and F.at(2, 5, 0) == 3 and F.at(0, -1, 0) < 0
    for s in (4, 6, 0):
        with pytest.raises(LookupError):
            F.at(0, s, 0)
    F.drop(5)
    with pytest.raises(LookupError):
        F.at(0, 5, 0)


def test_the_default_segment_length():
    assert seg_of(3452, 8) == 167 and seg_of(3452, 6) == 144 and seg_of(30344, 8) == 493  # ceil(sqrt((s' + 1) E))
    assert seg_of(0, 6) == 6 and seg_of(3, 6) == 6 and seg_of(35, 6) == 15 and seg_of(35, 1) == 6
    assert seg_of(10, 6, 1000) == 11 and seg_of(10, 6, 7) == 7 and seg_of(2, 6, 1000) == 6  # above the bound: one segment


def test_the_runs_stand_at_the_edges():
    """Over the runs of the new case lists under the models the gaps are made for: a found pair whose cost is a multiple of its seg, one
    at seg - 1 and one at 1 above a multiple, one below seg, one of more than ten segments, and segment boundaries crossed inside the
    insert layer and inside the delete layer."""
    SEEN.clear()
    for case in ("gaps", "small", "ladder"):
        for name in cases.GAP_MODELS + ("unit",):
            run_list(LISTS[case], name, False, False)
    multi = [x for x in SEEN if x[2] > 1]
    assert any(c % s == 0 for c, s, _, _ in multi)
    assert any(c % s == s - 1 for c, s, _, _ in multi)
    assert any(c % s == 1 and s > 2 for c, s, _, _ in multi)
    assert any(0 < c < s for c, s, _, _ in SEEN) and any(c == 0 for c, _, _, _ in SEEN)
    assert any(n > 10 for _, _, n, _ in SEEN)
    assert any(1 in cr for _, _, _, cr in SEEN) and any(2 in cr for _, _, _, cr in SEEN) and any(0 in cr for _, _, _, cr in SEEN)
    # the gaps: under affine(4, 6, 2) at seg = 8 the walk crosses ten boundaries inside the layer
    (a, b), (b2, a2) = cases.gaps()
    assert (a, b) == (a2, b2) and len(a) - len(b) == cases.GAP
    for name in cases.GAP_MODELS:
        d = affine_dt_seg(a, b, MODELS[name], BIG, 8)[4]
        i = affine_dt_seg(b, a, MODELS[name], BIG, 8)[4]
        assert d["crossed"].count(2) >= 4 and i["crossed"].count(1) >= 4, (name, d, i)
    assert affine_dt_seg(a, b, MODELS["affine"], BIG, 8)[4] == {"seg": 8, "nseg": 11, "crossed": [2] * 10}
    many = affine_dt_seg(*cases.many()[0], MODELS["affine"], BIG, 0)
    assert many[4]["nseg"] >= 5 and many[0] > 1000
    assert affine_dt_seg(*cases.many()[0], MODELS["affine"], many[0], 0)[4]["nseg"] > 10  # at its own cost as the bound, by default
