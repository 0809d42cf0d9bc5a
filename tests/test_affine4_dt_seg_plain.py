"""The plain segmented traceback of tests/affine4_dt_seg_plain.py against the plain double-affine diagonal transition of
tests/affine4_dt_plain.py: cost, start, end and CIGAR string are equal, over the pairs of tests/affine4_dt_seg_cases.py and the DT lists
that bear on the walk, under the three models of affine4_ends_cases.MODELS and STEEP, in the four ends settings, at five segment lengths
(Ew, Ew + 1, 2 Ew - 1, the default, one above every cost) and three bounds (none, the list's largest cost, that minus one).  The store
of the restatement is per ring and raises on a read outside the ring's h_r head rows and the segment, so every run is also a test of the
H-rows argument.  The last test asserts that the runs stood at the edges they are meant to cover."""
import pytest

from tests import affine4_dt_cases as dt4_cases
from tests import affine4_dt_seg_cases as cases
from tests import affine_dt_cases as dt_cases
from tests import affine_dt_ends_cases as ends_cases
from tests.affine4_dt_plain import affine4_dt
from tests.affine4_dt_seg_plain import E_of, Ew, H, _Ring, affine4_dt_seg, bound_of, heads, seg_of

MODELS = cases.MODELS
SETTINGS = ((False, False), (True, True), (True, False), (False, True))
BIG = (1 << 30) - 1
NOT_FOUND = (-1, -1, -1, "")
# (every gap length inside the pair, both directions; the gaps at the ends of the pair are the GPU test's)
LISTS = dict(cases.new_cases(), gaps=[p for x in range(0, len(dt4_cases.gaps()), 6) for p in dt4_cases.gaps()[x:x + 2]], tails=dt_cases.tails()[::9],
             tied=ends_cases.tied()[::2], two_piece=dt4_cases.two_piece(), ring_wraps=dt4_cases.ring_wraps()[:1], lengths=dt_cases.lengths()[::7],
             many=cases.many())
_ORACLE = {}
SEEN = []  # (model, cost, seg, nseg, crossed) of every found run, for the last test


def oracle(a, b, name, fs, fe):
    key = (a, b, name, fs, fe)
    if key not in _ORACLE:
        c, cig, st, en = affine4_dt(a, b, MODELS[name], BIG, fs, fe)
        _ORACLE[key] = (c, st, en, cig)
    return _ORACLE[key]


def segs_of(cm, top):
    w = Ew(cm)
    return (w, w + 1, max(2 * w - 1, w), 0, top + w + 1)


def run_list(pairs, name, fs, fe, segs=None):
    """Every pair at every seg without a bound, and under the two bounds every run in which the bound changes what the restatement
    computes.  The bound enters in two places only: through the segment length S (the default, and the cap max(Ew, s' + 1) on an
    explicit seg, which the length above every cost always meets) and through not finding a pair.  So a bounded run is left out
    exactly where the pair is found within the bound and S is the S of the unbounded run; it then repeats that run step for step."""
    cm = MODELS[name]
    want = [oracle(a, b, name, fs, fe) for a, b in pairs]
    top = max(w[0] for w in want)
    for s_max in (BIG, top, max(top - 1, 0)):
        for seg in segs or segs_of(cm, top):
            for (a, b), w in zip(pairs, want):
                n, m = len(a), len(b)
                if s_max != BIG and w[0] <= s_max and seg_of(bound_of(n, m, cm, s_max, fs, fe), cm, seg) == seg_of(bound_of(n, m, cm, BIG, fs, fe), cm, seg):
                    continue
                got = affine4_dt_seg(a, b, cm, s_max, seg, fs, fe)
                assert got[:4] == (w if w[0] <= s_max else NOT_FOUND), (len(a), len(b), s_max, seg)
                rec = got[4]
                assert rec["seg"] == seg_of(bound_of(len(a), len(b), cm, s_max, fs, fe), cm, seg)
                if got[0] >= 0:
                    assert rec["nseg"] == got[0] // rec["seg"] + 1 and len(rec["crossed"]) == rec["nseg"] - 1
                    SEEN.append((name, got[0], rec["seg"], rec["nseg"], tuple(rec["crossed"])))
                else:
                    assert rec["nseg"] == 0 and rec["crossed"] == []


PARAMS = [(name, s) for name in sorted(MODELS) for s in SETTINGS]


@pytest.mark.parametrize("name,setting", PARAMS, ids=["%s-fs%d-fe%d" % (n, *s) for n, s in PARAMS])
@pytest.mark.parametrize("case", sorted(set(LISTS) - {"many"}))
def test_results_equal_the_unsegmented_walk(case, name, setting):
    run_list(LISTS[case], name, *setting)


def test_the_2_kbp_pair_at_the_shortest_and_the_default_segment():
    # (one model and two segment lengths: the numpy oracle takes seconds a pair there)
    run_list(LISTS["many"], "double_affine", False, False, segs=(Ew(MODELS["double_affine"]), 0))


def test_the_store_raises_outside_the_head_and_the_segment():
    F = _Ring("0")
    F.put(5, 0, [1])
    assert F.at(5, 0) == 1 and F.at(-1, 0) < 0 and F.at(5, 3) < 0
    for s in (4, 6, 0):
        with pytest.raises(LookupError):
            F.at(s, 0)
    F.drop(5)
    with pytest.raises(LookupError):
        F.at(5, 0)


def test_the_rows_below_a_segment():
    d, s = MODELS["double_affine"], cases.STEEP
    assert heads(d) == (24, 2, 2, 1, 1) and (E_of(d), H(d), Ew(d)) == (24, 30, 24)
    assert heads(s) == (2, 9, 9, 8, 8) and (E_of(s), H(s), Ew(s)) == (2, 36, 9)  # Ew above E: the two-layer argument does not carry over
    assert heads(MODELS["asymmetric"]) == (20, 3, 2, 1, 1) and heads(MODELS["linear_edges"]) == (14, 2, 2, 1, 1)


def test_the_default_segment_length():
    d, s = MODELS["double_affine"], cases.STEEP
    # the smallest S with 5 S^2 >= (s' + 1) H, by hand: 3447 x 30 / 5 = 20682 and 143^2 = 20449 < 20682 <= 20736 = 144^2
    assert seg_of(3446, d) == 144
    assert seg_of(29999, d) == 425  # 30000 x 30 / 5 = 180000: 424^2 = 179776 < 180000 <= 425^2 = 180625
    assert seg_of(3332, d) == 142  # 3333 x 6 = 19998: 141^2 = 19881 < 19998 <= 142^2 = 20164
    assert seg_of(3455, d) == 144  # 3456 x 6 = 20736 = 144^2: equality is enough
    assert seg_of(3456, d) == 145  # 3457 x 6 = 20742 > 144^2
    assert seg_of(0, d) == 24 and seg_of(95, d) == 24 and seg_of(96, d) == 25  # raised to Ew while 5 x 24^2 = 2880 >= (s' + 1) 30
    assert seg_of(145, s) == 33  # 146 x 36 / 5 = 1051.2 -> 1052: 32^2 = 1024 < 1052 <= 1089 = 33^2
    assert seg_of(4, s) == 9 and seg_of(10, s) == 9  # 11 x 36 / 5 -> 80 <= 81
    assert seg_of(10, d, 1000) == 24 and seg_of(30, d, 1000) == 31 and seg_of(30, d, 25) == 25  # above the bound: one segment
    assert seg_of(3, s, 1000) == 9 and seg_of(20, s, 12) == 12


def test_the_runs_stand_at_the_edges():
    """Over the runs of the new case lists and the gaps: a found pair whose cost is a multiple of its seg, one at seg - 1 and one at 1
    above a multiple, one below seg, cost 0, one of more than ten segments, and segment boundaries crossed inside each of layers 1, 2,
    3 and 4 and on the main layer."""
    SEEN.clear()
    for case in ("long_gap", "small", "ladder"):
        for name in sorted(MODELS):
            run_list(LISTS[case], name, False, False)
    run_list(LISTS["gaps"], "double_affine", False, False)
    multi = [x for x in SEEN if x[3] > 1]
    assert any(c % s == 0 for _, c, s, _, _ in multi)
    assert any(c % s == s - 1 for _, c, s, _, _ in multi)
    assert any(c % s == 1 and s > 2 for _, c, s, _, _ in multi)
    assert any(0 < c < s for _, c, s, _, _ in SEEN) and any(c == 0 for _, c, _, _, _ in SEEN)
    assert any(n > 10 for _, _, _, n, _ in SEEN)
    for layer in range(5):
        assert any(layer in cr for _, _, _, _, cr in SEEN), layer
    # under double_affine at seg = 24: the 18-byte gap on the first piece, the 100-byte gap on the second
    d = MODELS["double_affine"]
    (da, db), (ia, ib) = cases.gap18()
    assert len(da) - len(db) == 18 and len(ib) - len(ia) == 18
    assert affine4_dt_seg(da, db, d, BIG, 24)[::4] == (42, {"seg": 24, "nseg": 2, "crossed": [2]})
    assert affine4_dt_seg(ia, ib, d, BIG, 24)[::4] == (42, {"seg": 24, "nseg": 2, "crossed": [1]})
    (da, db), (ia, ib) = cases.long_gap()
    assert affine4_dt_seg(da, db, d, BIG, 24)[::4] == (124, {"seg": 24, "nseg": 6, "crossed": [4, 4, 4, 4, 0]})
    assert affine4_dt_seg(ia, ib, d, BIG, 24)[::4] == (124, {"seg": 24, "nseg": 6, "crossed": [3, 3, 3, 3, 0]})
    # under STEEP, Ew = 9 > E = 2: sixteen boundaries inside the layer, at a segment length the main layer alone would not ask for
    (da, db), (ia, ib) = cases.gap18()
    assert affine4_dt_seg(da, db, cases.STEEP, BIG, 9)[::4] == (146, {"seg": 9, "nseg": 17, "crossed": [4] * 16})
    assert affine4_dt_seg(ia, ib, cases.STEEP, BIG, 9)[::4] == (146, {"seg": 9, "nseg": 17, "crossed": [3] * 16})
    with pytest.raises(AssertionError):
        affine4_dt_seg(da, db, cases.STEEP, BIG, 8)  # below Ew: refused


def test_a_segment_below_Ew_breaks_the_argument():
    """S = 8 under STEEP, where E = 2 would allow it and Ew = 9 does not, run unchecked: the fill of a segment asks a layer's ring for
    the front nine costs back, which lies below the eight-cost segment before it, and the store raises.  Under double_affine S = 23
    fails in the main ring likewise.  At S = Ew the same pairs pass (above)."""
    for a, b in cases.gap18():
        for seg in (8, 7, 2):
            with pytest.raises(LookupError, match=r"is not in ring [1-4]"):
                affine4_dt_seg(a, b, cases.STEEP, BIG, seg, unchecked=True)
        assert affine4_dt_seg(a, b, cases.STEEP, BIG, 9, unchecked=True)[0] == 146
    a, b = cases.long_gap()[0]
    with pytest.raises(LookupError, match="is not in ring 0"):
        affine4_dt_seg(a, b, MODELS["double_affine"], BIG, 23, unchecked=True)
