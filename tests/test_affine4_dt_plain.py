"""The plain four-layer diagonal transition of tests/affine4_dt_plain.py against independent statements, without a GPU: the layered NW
of tests/affine4_plain.py (global cost), the ends-free DP of tests/affine4_ends_plain.py (cost and end under the four settings), the
CIGAR pricer affine4_verify over a[start:end], the two-layer oracles of tests/affine_dt_plain.py / affine_dt_ends_plain.py with layers 2
and 3 priced out of reach (cost and CIGAR), the known answers at the crossover of the two pieces, and not found exactly at cost - 1;
over seeded pairs and the lists of tests/affine4_dt_cases.py under the three models of affine4_ends_cases.MODELS.  And the case lists are
what they claim to be."""
import numpy as np
import pytest

from astar_pairwise_aligner_amd import AffineCost
from tests import affine4_dt_cases as cases
from tests import affine_plain as ap
from tests.affine4_dt_plain import affine4_dt, del_cost, ins_cost, mean_w
from tests.affine4_ends_plain import affine4_ends
from tests.affine4_plain import _model, affine4_nw, affine4_verify
from tests.affine_dt_ends_plain import affine_dt_ends
from tests.affine_dt_plain import affine_dt
from tests.affine_ends_cases import mutate, rand_seq

MODELS = cases.MODELS
GLOBAL = cases.global_cases()
ENDS = cases.ends_cases_all()
BIG = (1 << 30) - 1
NOT_FOUND = (-1, "", -1, -1)


def thin(case, pairs, name, setting=(False, False)):
    """A third of the lists of more than 60 pairs per model, another third for another model; under the ends-free settings a sixth,
    another one per setting."""
    if len(pairs) <= 60:
        return pairs
    step = 6 if setting != (False, False) else 3
    return pairs[(len(name) + 2 * setting[0] + setting[1]) % step::step]


def seeded(seed, count=12):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = rand_seq(rng, int(rng.integers(0, 120)))
        b = mutate(rng, a, float(rng.choice([0.02, 0.1, 0.3]))) if rng.random() < 0.7 else rand_seq(rng, int(rng.integers(0, 120)))
        out.append((a, b))
    return out


def check_global(pairs, cm):
    for p, (a, b) in enumerate(pairs):
        want = affine4_nw(a, b, cm, trace=False)[0]
        cost, cigar, start, end = affine4_dt(a, b, cm, BIG)
        assert (cost, start, end) == (want, 0, len(a)), (p, len(a), len(b))
        assert affine4_verify(cigar, a, b, cm) == cost and ap.no_adjacent_same_op(cigar), (p, cigar)
        assert affine4_dt(a, b, cm, cost) == (cost, cigar, start, end)
        if cost > 0:
            assert affine4_dt(a, b, cm, cost - 1) == NOT_FOUND


@pytest.mark.parametrize("case,name", [(c, n) for c in sorted(GLOBAL) for n in cases.models_of(c)])
def test_global_cost_is_the_layered_nw_s(case, name):
    check_global(thin(case, GLOBAL[case], name), MODELS[name])


@pytest.mark.parametrize("name", sorted(MODELS))
def test_global_on_seeded_pairs(name):
    check_global(seeded(41), MODELS[name])


def check_ends(pairs, cm, fs, fe):
    for p, (a, b) in enumerate(pairs):
        want_cost, _, want_end, _, _ = affine4_ends(a, b, cm, fs, fe, trace=False)
        got = affine4_dt(a, b, cm, BIG, fs, fe)
        cost, cigar, start, end = got
        assert (cost, end) == (want_cost, want_end), (p, len(a), len(b))
        assert 0 <= start <= end <= len(a) and (fs or start == 0) and (fe or end == len(a))
        assert affine4_verify(cigar, a[start:end], b, cm) == cost and ap.no_adjacent_same_op(cigar), (p, cigar)
        if cost > 0:
            assert affine4_dt(a, b, cm, cost - 1, fs, fe) == NOT_FOUND
        else:
            assert affine4_dt(a, b, cm, 0, fs, fe) == got


# all four settings under double_affine, both ends free under the other two models (tests/test_gpu_affine4_dt.py runs the same)
ENDS_PARAMS = [(c, n, s) for c in sorted(ENDS) for n in cases.models_of(c) for s in cases.SETTINGS if n == "double_affine" or s == (True, True)]


@pytest.mark.parametrize("case,name,setting", ENDS_PARAMS, ids=["%s-%s-fs%d-fe%d" % (c, n, *s) for c, n, s in ENDS_PARAMS])
def test_ends_free_cost_and_end_are_the_plain_dp_s(case, name, setting):
    check_ends(thin(case, ENDS[case], name, setting), MODELS[name], *setting)


@pytest.mark.parametrize("setting", cases.SETTINGS, ids=lambda s: "fs%d-fe%d" % s)
def test_ends_free_on_seeded_pairs(setting):
    rng = np.random.default_rng(43)
    pairs = []
    for _ in range(8):
        y = rand_seq(rng, int(rng.integers(10, 70)))
        pairs.append((rand_seq(rng, int(rng.integers(0, 40))) + mutate(rng, y, 0.1) + rand_seq(rng, int(rng.integers(0, 40))), y))
    for name in sorted(MODELS):
        check_ends(pairs, MODELS[name], *setting)


def test_layers_out_of_reach_give_the_two_layer_oracle_cost_and_cigar():
    """Layers 2 and 3 at open = 1000 never pay for themselves on pairs this short, and the parents of layers 0 and 1 keep their places
    in the order: the CIGAR is the two-layer walk's."""
    four = AffineCost(4, None, None, [("ins", 6, 2), ("del", 6, 2), ("ins", 1000, 1), ("del", 1000, 1)])
    two = AffineCost.affine(4, 6, 2)
    four_lin = AffineCost(3, 5, 4, [("ins", 4, 2), ("del", 3, 2), ("ins", 1000, 1), ("del", 1000, 1)])
    two_lin = AffineCost(3, 5, 4, [("ins", 4, 2), ("del", 3, 2)])
    pairs = seeded(44) + GLOBAL["gaps"][::7] + GLOBAL["low_complexity"] + GLOBAL["tails"][::9]
    for c4, c2 in ((four, two), (four_lin, two_lin)):
        for a, b in pairs:
            cost, cigar = affine_dt(a, b, c2, BIG)
            assert affine4_dt(a, b, c4, BIG) == (cost, cigar, 0, len(a))
    windows = ENDS["tied"] + ENDS["flanked"][::4] + ENDS["gaps"][::9]
    for fs, fe in cases.SETTINGS:
        for a, b in windows:
            cost, start, end, cigar = affine_dt_ends(a, b, two, BIG, fs, fe)
            assert affine4_dt(a, b, four, BIG, fs, fe) == (cost, cigar, start, end)


def test_known_answers_at_the_crossover():
    """Under double_affine(4, 6, 2, 24, 1) a gap of 18 costs 6 + 36 = 42 on either piece and a gap of 19 costs 24 + 19 = 43."""
    cm = cases.DOUBLE
    x = b"ACGTTGCAAGCTTAGCCGATATCGGCTAAC"
    for L, want in ((17, 40), (18, 42), (19, 43), (20, 44), (40, 64)):
        g = b"K" * L
        for a, b, op in ((x[:15] + g + x[15:], x, "D"), (x, x[:15] + g + x[15:], "I")):
            assert affine4_dt(a, b, cm, BIG) == (want, "15=%d%s15=" % (L, op), 0, len(a))
            assert affine4_dt(a, b, cm, want - 1) == NOT_FOUND
        assert affine4_dt(g + x, x, cm, BIG, True, False) == (0, "30=", L, L + 30)
        assert affine4_dt(x + g, x, cm, BIG, False, True) == (0, "30=", 0, 30)
        assert affine4_dt(x, g + x, cm, BIG, True, True) == (want, "%dI30=" % L, 0, 30)
    assert cases.SECOND_PIECE_FROM == 19 and ins_cost(18, cm) == 42 and del_cost(19, cm) == 43
    assert affine4_dt(b"", b"", cm, 0) == (0, "", 0, 0)
    assert affine4_dt(b"ACGT", b"", cm, BIG) == (14, "4D", 0, 4) and affine4_dt(b"", b"ACGT", cm, 13) == NOT_FOUND


def test_the_case_lists_are_worth_running():
    cm = cases.DOUBLE
    # gaps: every length, both directions, three places; the cost is one gap's, on the piece the length asks for
    assert len(GLOBAL["gaps"]) == 6 * len(cases.GAP_LENGTHS) and {17, 18, 19, 20, 40} <= set(cases.GAP_LENGTHS)
    for x, (a, b) in enumerate(GLOBAL["gaps"]):
        L = cases.GAP_LENGTHS[x // 6]
        assert abs(len(a) - len(b)) == L
        for name in sorted(MODELS):
            want = del_cost(L, MODELS[name]) if len(a) > len(b) else ins_cost(L, MODELS[name])
            assert affine4_dt(a, b, MODELS[name], BIG)[0] == want, (x, name)
    # the crossovers the lengths stand on: the first length at which the second piece is strictly cheaper
    def first(c, t):  # layer t + 2 against layer t
        _, _, _, op, ex = _model(c)
        return next(L for L in range(1, 100) if op[t + 2] + L * ex[t + 2] < op[t] + L * ex[t])

    assert [first(MODELS[n], 0) for n in ("double_affine", "asymmetric", "linear_edges")] == [19, 7, 9]
    assert [first(MODELS[n], 1) for n in ("double_affine", "asymmetric", "linear_edges")] == [19, 14, 12]
    assert all(L - 1 in cases.GAP_LENGTHS and L in cases.GAP_LENGTHS for L in (19, 7, 9, 14, 12))
    # ring_wraps: several wraps of the deepest ring (25 slots) and so many more of the shallowest (2)
    assert all(affine4_dt(a, b, cm, BIG)[0] > 4 * 25 for a, b in GLOBAL["ring_wraps"])
    # wide and narrow blocks
    top = max(affine4_dt(a, b, cm, BIG)[0] for a, b in GLOBAL["mixed"])
    for s_max in (BIG, top, top - 1):
        assert mean_w(GLOBAL["mixed"], cm, s_max) > cases.WIDE_MEAN
    assert sorted(len(a) for a, _ in GLOBAL["mixed"])[-2:] == [2100, 2900]
    for name in ("far_diagonals", "wide"):  # under an extend of 1 the bound of an unrelated pair pays for nearly every diagonal
        assert mean_w(GLOBAL[name], cm, BIG) > cases.WIDE_MEAN
    for name in sorted(set(GLOBAL) - {"mixed", "far_diagonals", "wide"}):
        assert mean_w(GLOBAL[name], cm, BIG) <= cases.WIDE_MEAN, name
    for name in ("windows", "long"):
        assert mean_w(ENDS[name], cm, BIG, True, True) > cases.WIDE_MEAN, name
    for name in ("tied", "lengths", "tails", "gaps"):
        assert mean_w(ENDS[name], cm, BIG, True, True) <= cases.WIDE_MEAN, name
    # the DT walk and the DP walk differ somewhere: the CIGAR is the oracle's own
    other = sum(affine4_dt(a, b, cm, BIG)[1] != affine4_nw(a, b, cm)[1] for a, b in GLOBAL["low_complexity"] + GLOBAL["wide"][:3])
    assert other >= 1
