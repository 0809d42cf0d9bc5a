"""The plain diagonal transition of tests/affine_dt_plain.py against the plain NW of tests/affine_plain.py, over the pairs of
tests/affine_dt_cases.py and all seven model constructors: same cost, a CIGAR that prices to it, found at s_max = cost and not found at
cost - 1, and the case lists are what they claim to be."""
import pytest

from tests import affine_dt_cases as cases
from tests import affine_plain as ap
from tests.affine_dt_plain import affine_dt, reach

MODELS = cases.MODELS
CASES = cases.all_cases()
BIG = (1 << 30) - 1


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_cost_and_cigar_equal_the_plain_nw(case, name):
    cm = MODELS[name]
    pairs = CASES[case]
    if case == "mixed" and name not in ("affine", "unit"):
        pairs = [p for p in pairs if len(p[0]) < 1000]  # (the plain NW takes a second per long pair; two models carry them)
    if case == "lengths":
        pairs = pairs[len(name) % 3::3]  # (a third of the 196 per model, another third for another model)
    for a, b in pairs:
        want = ap.affine_nw(a, b, cm, trace=False)[0]
        cost, cigar = affine_dt(a, b, cm, want)
        assert cost == want, (len(a), len(b))
        assert ap.affine_verify(cigar, a, b, cm) == cost and ap.no_adjacent_same_op(cigar)
        assert affine_dt(a, b, cm, BIG) == (cost, cigar)  # the bound does not change what is found
        if cost > 0:
            assert affine_dt(a, b, cm, cost - 1) == (-1, "")
        if a == b:
            assert (cost, cigar) == (0, f"{len(a)}=" if len(a) > 1 else "=" * len(a))


def test_equal_sequences():
    for n in (0, 1, 2, 8, 9, 100):
        a = bytes(range(n))
        assert affine_dt(a, a, MODELS["affine"], 0) == (0, "" if n == 0 else "=" if n == 1 else f"{n}=")


def test_the_case_lists_are_what_they_claim():
    cm = MODELS["affine"]
    L = cases.LENGTHS
    assert {(len(a), len(b)) for a, b in CASES["lengths"]} == {(n, m) for n in L for m in L}
    assert any(a == b and len(a) > 8 for a, b in CASES["tails"])
    assert {len(a) - len(b) for a, b in CASES["far_diagonals"]} == {70, -70, 130, -130}
    # the fronts of the unrelated pairs grow past 128 diagonals, and the ring of affine(4, 6, 2), 7 fronts, wraps many times
    sub, ins, dl, io, ie, do, de = ap.edge_costs(cm)
    widths = []
    for a, b in CASES["wide"]:
        c = affine_dt(a, b, cm, BIG)[0]
        assert c > 10 * 7
        widths.append(min(len(b), reach(c, ins, io, ie)) + min(len(a), reach(c, dl, do, de)) + 1)
    assert max(widths) > 128 and min(widths) > 64
    long_ = [(a, b) for a, b in CASES["mixed"] if len(a) > 2000]
    assert len(long_) == 2 and all(2000 <= len(b) <= 3300 for _, b in long_)
    for a, b in long_:
        c = affine_dt(a, b, cm, BIG)[0]
        assert 0.05 * len(a) * 4 < c < 0.2 * len(a) * 8  # about 10 %


def test_walk_rule_prefers_substitution_then_insert_then_delete():
    # AC / CA under unit costs: XX (2) ties with I=D / D=I; the walk takes the substitution first
    assert affine_dt(b"AC", b"CA", MODELS["unit"], 5) == (2, "2X")
    # one extra byte in b between equal halves, under a model with both a linear and an affine insert
    assert affine_dt(b"ACGTACGT", b"ACGTTACGT", MODELS["linear_affine"], 9) == (2, "4=I4=")
