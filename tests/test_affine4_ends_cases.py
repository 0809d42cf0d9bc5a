"""The pairs of tests/affine4_ends_cases.py are worth running: asked of the plain DP alone, under free_start = free_end = 1 and
double_affine(4, 6, 2, 24, 1), they hold hits away from both ends of the text, tied last-row minima, ends at column 0 and at |a|; and
the CIGARs of two_piece() really contain the second-piece gaps they were built for, where they were built to be."""
import pytest

from tests import affine4_ends_cases as cases
from tests.affine4_ends_plain import affine4_ends
from tests.affine_plain import cigar_elems

CM = cases.DOUBLE
R = cases.R


def runs(cigar, op):
    return [k for k, o in cigar_elems(cigar) if o == op]


@pytest.fixture(scope="module")
def answers():
    named = {"edge0": cases.edge_pairs(0), "flanked": cases.flanked(), "packed_unequal": cases.packed_unequal(), "two_piece": cases.two_piece()}
    return {name: [(x, y) + affine4_ends(x, y, CM, True, True) for x, y in pairs] for name, pairs in named.items()}


def test_rows_per_lane_are_those_of_the_two_layer_batch():
    from astar_pairwise_aligner_amd.capi import AFFINE_ROWS_PER_LANE
    assert R == AFFINE_ROWS_PER_LANE == 16


def test_the_cases_are_not_trivial(answers):
    every = [r for rs in answers.values() for r in rs]
    inside = sum(0 < start and end < len(x) for x, _, _, start, end, _, _ in every)
    assert 3 * inside >= len(every), (inside, len(every))
    assert any(int((row == row.min()).sum()) >= 2 for *_, row in every)
    assert any(end == 0 and len(x) > 0 for x, _, _, _, end, _, _ in every)
    assert any(end == len(x) > 0 for x, _, _, _, end, _, _ in every)
    x, y, cost, start, end, _, row = next(r for r in answers["flanked"] if r[0] == r[1] + r[1])
    assert (cost, start, end) == (0, 0, len(y)) and row[2 * len(y)] == 0  # tied at two ends: the lower one is the answer


def test_two_piece_cases_hold_second_piece_gaps(answers):
    rs = answers["two_piece"]
    assert len(rs) == 4
    for x, y, cost, start, end, cigar, _ in rs:
        assert 0 < start and end < len(x)
        assert max(runs(cigar, "I") + runs(cigar, "D")) >= cases.SECOND_PIECE_FROM
    # 0: 30 columns deleted, columns 56 .. 85 of the text: the run crosses column 64
    x, y, cost, start, end, cigar, _ = rs[0]
    (k0, o0), (k1, o1), (k2, o2) = cigar_elems(cigar)  # (where the run begins may slide over bytes that repeat)
    assert (cost, start, end) == (24 + 30, 20, 120) and (o0, k1, o1, o2) == ("=", 30, "D", "=") and start + k0 < 64 < start + k0 + 30
    # 1: 40 rows inserted, rows 64 R - 23 .. 64 R + 16
    x, y, cost, start, end, cigar, _ = rs[1]
    assert (cost, start, end, cigar) == (24 + 40, 30, 30 + 64 * R + 100, f"{64 * R - 24}=40I124=")
    # 2: the pattern's first 40 rows inserted: the walk comes to row 0 inside the second insert layer
    x, y, cost, start, end, cigar, _ = rs[2]
    assert (cost, start, end, cigar) == (24 + 40, 45, 145, "40I100=")
    # 3: the end 24 columns after a deletion run of 20, which only the second piece makes cheaper than inserting the tail
    x, y, cost, start, end, cigar, row = rs[3]
    assert (cost, start, end, cigar) == (24 + 20, 30, 124, "50=20D24=")
    assert 6 + 2 * 20 > cost and min(6 + 2 * 24, 24 + 24) > cost  # the first piece would pay more for the run; so would inserting the tail
    assert int(row[80]) > cost  # ending before the deletion is worse
