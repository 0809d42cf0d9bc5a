"""The plain ends-free diagonal transition of tests/affine_dt_ends_plain.py against the plain ends-free DP of tests/affine_ends_plain.py,
over the pairs of tests/affine_dt_ends_cases.py, the four settings, and SETTING_MODELS plus unit: same cost and end, a CIGAR that prices
to the cost over a[start:end], affine_dt with both switches off, not found at cost - 1; and the case lists are what they claim to be."""
import pytest

from tests import affine_dt_ends_cases as cases
from tests import affine_plain as ap
from tests.affine_dt_ends_plain import affine_dt_ends
from tests.affine_dt_plain import affine_dt, gap_cost, reach
from tests.affine_ends_plain import affine_ends

MODELS = cases.MODELS
CASES = cases.all_cases()
NAMES = cases.SETTING_MODELS + ("unit",)
BIG = (1 << 30) - 1


@pytest.mark.parametrize("setting", cases.SETTINGS, ids=lambda s: "fs%d-fe%d" % s)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_cost_and_end_equal_the_plain_dp(case, name, setting):
    cm = MODELS[name]
    fs, fe = setting
    pairs = CASES[case]
    if case == "lengths":
        pairs = pairs[len(name) % 3::3]  # (a third of the 196 per model, another third for another model)
    for p, (a, b) in enumerate(pairs):
        cost, _, end, _, _ = affine_ends(a, b, cm, fs, fe, trace=False)
        got = affine_dt_ends(a, b, cm, BIG, fs, fe)
        assert got[0] == cost and got[2] == end, (p, len(a), len(b))
        c, start, end, cigar = got
        assert 0 <= start <= end <= len(a) and (fs or start == 0) and (fe or end == len(a))
        assert ap.affine_verify(cigar, a[start:end], b, cm) == cost and ap.no_adjacent_same_op(cigar)
        if cost > 0:
            assert affine_dt_ends(a, b, cm, cost - 1, fs, fe) == (-1, -1, -1, "")
        else:
            assert affine_dt_ends(a, b, cm, 0, fs, fe) == got
        if not fs and not fe:
            assert (c, cigar) == affine_dt(a, b, cm, BIG)


def test_the_case_lists_are_worth_running():
    cm = MODELS["affine"]
    inner = tie = end0 = short = other = 0
    for name in sorted(CASES):
        for a, b in CASES[name]:
            cost, start, end, cigar, row = affine_ends(a, b, cm, True, True)
            got = affine_dt_ends(a, b, cm, BIG, True, True)
            inner += got[1] > 0 and got[2] < len(a)
            tie += int((row == cost).sum()) > 1
            end0 += end == 0
            short += len(a) < len(b)
            other += got[3] != cigar
    assert inner >= 5 and tie >= 1 and end0 >= 1 and short >= 1 and other >= 1, (inner, tie, end0, short, other)


def test_the_new_lists_stand_at_the_kernel_edges():
    cm = MODELS["affine"]
    sub, ins, dl, io, ie, do, de = ap.edge_costs(cm)
    y8, y = CASES["tied"][0]
    assert len(y) == 40 and y8 == y * 8
    row = affine_ends(y8, y, cm, True, True, trace=False)[4]
    assert [i for i, v in enumerate(row) if v == 0] == list(range(40, 321, 40))
    assert affine_dt_ends(y8, y, cm, 0, True, True) == (0, 0, 40, "40=")
    assert affine_dt_ends(y8, y, cm, 0, False, True) == (0, 0, 40, "40=")
    assert affine_dt_ends(y8, y, cm, BIG, True, False) == (0, 280, 320, "40=")
    assert affine_dt_ends(*CASES["tied"][1], cm, BIG, True, True)[0] > 0
    assert affine_dt_ends(*CASES["tied"][4], cm, 0, True, True) == (0, 0, 0, "")
    assert {len(a) for a, b in CASES["windows"][8:]} == set(cases.WINDOW_TEXTS) and all(len(b) == 100 for a, b in CASES["windows"][8:])
    assert all(len(a) == 400 and len(b) == 150 for a, b in CASES["windows"][:8])

    def mean_w(pairs, s_max):
        """The mean W of a batch under free_start by the host's rule (kmax = min(|a|, |a| - |b| + reach_ins(s')), W = kmax - kmin + 3);
        its blocks are wide where this exceeds 256."""
        ws = []
        for a, b in pairs:
            n, m = len(a), len(b)
            back = reach(min(s_max, gap_cost(m, ins, io, ie)), ins, io, ie)
            ws.append(min(n, max(0, n - m + back)) + min(m, back) + 3)
        return sum(ws) / len(ws)

    def top(pairs):
        return max(affine_dt_ends(a, b, cm, BIG, True, True)[0] for a, b in pairs)

    for name in ("windows", "long"):  # wide at the bounds the GPU test takes above 0: unbounded, the largest cost, that minus one
        for s_max in (BIG, top(CASES[name]), top(CASES[name]) - 1):
            assert mean_w(CASES[name], s_max) > 256, (name, s_max)
    assert mean_w(CASES["tied"][:2] + CASES["windows"], BIG) > 256  # (tests/test_gpu_affine_dt_ends.py: tied ends across wavefronts)
    for name in ("tied", "lengths", "tails", "packed_unequal"):
        assert mean_w(CASES[name], BIG) <= 256, name
    (a, b), (a2, b2) = CASES["long"]
    assert (len(a), len(b), len(b2)) == (2500, 2100, 60)
    c = affine_dt_ends(a, b, cm, BIG, True, True)[0]
    assert c > 20 * 7  # the ring of affine(4, 6, 2), 7 fronts, wraps many times
