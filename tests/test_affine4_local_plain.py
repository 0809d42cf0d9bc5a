"""The double-affine local-alignment oracle (tests/affine4_local_plain.py) against a brute force that goes through the global oracle
(tests/affine4_plain.py), against the two-layer local oracle where both pieces are equal, and its own invariants on seeded random pairs.

The brute force: for every s <= e, t <= u the doubled score of the best alignment of a[s:e] with b[t:u] is
    match * ((e - s) + (u - t)) - affine4_nw(a[s:e], b[t:u], cm'')
where cm'' has sub'' = 2 sub + 2 match, ins'' = 2 ins + match (del'' likewise), open_k'' = 2 open_k, extend_k'' = 2 extend_k + match:
every byte an alignment consumes is paid match / 2 in advance, a match keeps it, and every other edge pays it back on top of twice its
cost.  The local score is the maximum over all (s, e, t, u), halved, and never below 0.
"""
import numpy as np
import pytest

from astar_pairwise_aligner_amd import AffineCost
from tests import affine4_local_plain as lp4
from tests import affine4_plain as a4
from tests import affine_local_plain as lp
from tests import affine_plain as ap
from tests.test_gpu_affine4 import MODELS

BRUTE_MATCH = {"double_affine": 2, "linear_edges": 3, "no_sub": 1, "asymmetric": 2}
DOUBLE = MODELS["double_affine"]


def doubled(cm, match):
    d = lambda v: None if v is None else 2 * v + match  # noqa: E731
    return AffineCost(None if cm.sub is None else 2 * cm.sub + 2 * match, d(cm.ins), d(cm.del_), [(k, 2 * o, 2 * e + match) for k, o, e in cm.layers])


def brute(a, b, cm, match):
    cm2 = doubled(cm, match)
    best = 0
    for s in range(len(a) + 1):
        for e in range(s, len(a) + 1):
            for t in range(len(b) + 1):
                for u in range(t, len(b) + 1):
                    best = max(best, match * ((e - s) + (u - t)) - a4.affine4_nw(a[s:e], b[t:u], cm2, trace=False)[0])
    assert best % 2 == 0
    return best // 2


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_oracle_against_the_global_oracle(name):
    cm, match = MODELS[name], BRUTE_MATCH[name]
    rng = np.random.default_rng(200 + len(name))
    for _ in range(12):
        a, b = rand_seq(rng, int(rng.integers(0, 7)), b"AC"), rand_seq(rng, int(rng.integers(0, 7)), b"AC")
        score, cigar, a0, a1, b0, b1 = lp4.local_sw4(a, b, cm, match)
        assert score == brute(a, b, cm, match), (a, b)
        assert cigar == "" or (cigar[-1] == "=" and ap.cigar_elems(cigar)[0][1] == "=")


@pytest.mark.parametrize("soe", ((4, 6, 2), (1, 1, 1), (3, 9, 1)))
def test_equal_pieces_agree_with_the_two_layer_oracle(soe):
    s, o, e = soe
    cm4, cm2 = AffineCost.double_affine(s, o, e, o, e), AffineCost.affine(s, o, e)
    rng = np.random.default_rng(sum(soe))
    for k in range(30):
        n, m = int(rng.integers(0, 61)), int(rng.integers(0, 61))
        alphabet = b"ACGT" if k % 2 else b"AC"
        a, b = rand_seq(rng, n, alphabet), rand_seq(rng, m, alphabet)
        match = (1, 2, 5, 1000)[k % 4]
        assert lp4.local_sw4(a, b, cm4, match) == lp.local_sw(a, b, cm2, match), (a, b, match)


def check_one(a, b, cm, match):
    score, cigar, a0, a1, b0, b1 = lp4.local_sw4(a, b, cm, match)
    assert lp4.local_sw4(a, b, cm, match, trace=False) == (score, None, None, a1, None, b1)
    if score == 0:
        assert (cigar, a0, a1, b0, b1) == ("", 0, 0, 0, 0)
        return
    assert 0 <= a0 < a1 <= len(a) and 0 <= b0 < b1 <= len(b)
    assert lp4.local_verify4(cigar, a, b, a0, b0, cm, match) == (score, a1, b1)  # the price, and the endpoints by the CIGAR's lengths
    elems = ap.cigar_elems(cigar)
    assert elems[0][1] == "=" and elems[-1][1] == "="


@pytest.mark.parametrize("name", sorted(MODELS))
def test_invariants_on_seeded_random_pairs(name):
    rng = np.random.default_rng(len(name) * 11)
    cm = MODELS[name]
    for k in range(40):
        n, m = int(rng.integers(0, 61)), int(rng.integers(0, 61))
        alphabet = b"ACGT" if k % 2 else b"AC"
        check_one(rand_seq(rng, n, alphabet), rand_seq(rng, m, alphabet), cm, (1, 2, 5, 1000)[k % 4])


def test_score_zero_is_the_empty_alignment():
    for a, b in ((b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"GGTT", b"ACCA")):
        assert lp4.local_sw4(a, b, DOUBLE, 2) == (0, "", 0, 0, 0, 0)


def test_planted_ties_take_the_lowest_i_then_the_lowest_j():
    w = b"ACCA"
    # the same i, two j: the lower j
    assert lp4.local_sw4(b"GG" + w, w + b"TT" + w, DOUBLE, 3) == (12, "4=", 2, 6, 0, 4)
    # two i, the higher j at the lower i: the lower i
    assert lp4.local_sw4(w + b"GG" + w, b"T" + w, DOUBLE, 3) == (12, "4=", 0, 4, 1, 5)
    assert lp4.local_sw4(w + b"GGG" + w, w + b"TTTTTTTTTT" + w, DOUBLE, 3) == (12, "4=", 0, 4, 0, 4)
    # two words of one score, (i, j) = (4, 18) against (11, 4): the lower i wins although its j is higher
    v = b"CAAC"
    assert lp4.local_sw4(w + b"GGG" + v, v + b"TTTTTTTTTT" + w, DOUBLE, 3) == (12, "4=", 0, 4, 14, 18)


W1 = bytes(range(0x80, 0x80 + 50))  # two 50-byte words over bytes that occur nowhere else (none of ACGT)
W2 = bytes(range(0xC0, 0xC0 + 50))


def gap_pair(rng, in_b: bool):
    """Two words next to each other in one sequence and 60 bytes apart in the other, nothing else in common."""
    joined = rand_seq(rng, 7, b"GT") + W1 + W2 + rand_seq(rng, 9, b"GT")
    split = rand_seq(rng, 5, b"AC") + W1 + rand_seq(rng, 60, b"AC") + W2 + rand_seq(rng, 4, b"AC")
    return (joined, split) if in_b else (split, joined)


@pytest.mark.parametrize("in_b", (True, False))
def test_a_gap_only_the_second_piece_affords(in_b):
    a, b = gap_pair(np.random.default_rng(3), in_b)
    op = "I" if in_b else "D"
    # the second piece pays 24 + 60 * 1 = 84 of the words' 200 and joins them; the first alone would pay 6 + 60 * 2 = 126: 74 < 100
    sa, sb = (7, 5) if in_b else (5, 7)
    assert lp4.local_sw4(a, b, AffineCost.double_affine(4, 6, 2, 24, 1), 2) == (116, f"50=60{op}50=", sa, sa + (100 if in_b else 160), sb, sb + (160 if in_b else 100))
    assert lp4.local_sw4(a, b, AffineCost.double_affine(4, 6, 2, 6, 2), 2) == (100, "50=", sa, sa + 50, sb, sb + 50)


def test_a_bad_match_is_refused():
    for bad in (True, 1.5, "2", None, 0, 1001):
        with pytest.raises(ValueError, match="match"):
            lp4.local_sw4(b"AC", b"AC", DOUBLE, bad)
