"""The pairs of tests/affine_ends_cases.py are worth running: asked of the plain DP alone, under free_start = free_end = 1 and
affine(4, 6, 2), they hold hits away from both ends of the text, a tied last-row minimum, ends at column 0 and at |a|, texts shorter
than their pattern and empty texts; the packed wavefront's short texts end at their own |a|; and the tile-edge hits start and end on and
next to the tile edges."""
import numpy as np
import pytest

from tests import affine_ends_cases as cases
from tests import affine_plain as ap
from tests.affine_ends_plain import affine_ends

CM = cases.MODELS["affine"]


@pytest.fixture(scope="module")
def answers():
    return {name: [(x, y) + affine_ends(x, y, CM, True, True) for x, y in pairs] for name, pairs in cases.all_cases(rots=(0,)).items()}


def test_the_cases_are_not_trivial(answers):
    every = [r for rs in answers.values() for r in rs]
    inside = sum(0 < start and end < len(x) for x, _, _, start, end, _, _ in every)
    assert 3 * inside >= len(every), (inside, len(every))
    assert any(int((row == row.min()).sum()) >= 2 for *_, row in every)
    assert any(end == 0 and len(x) > 0 for x, _, _, _, end, _, _ in every)
    assert any(end == len(x) > 0 for x, _, _, _, end, _, _ in every)
    assert any(len(x) < len(y) for x, y, *_ in every) and any(len(x) == 0 for x, *_ in every)
    x, y, cost, start, end, _, row = next(r for r in answers["flanked"] if r[0] == r[1] + r[1])
    assert (cost, start, end) == (0, 0, len(y)) and row[2 * len(y)] == 0  # tied at two ends: the lower one is the answer


def test_edge_shapes_cover_every_pattern_and_text_length():
    seen = {(len(y), len(x)) for x, y in cases.edge_all()}
    assert len(cases.edge_all()) == 45  # (|b| = 0 and 1 meet |a| = 0 more than once)
    assert seen == {(m, n) for m in cases.EDGE_M for n in cases.edge_n(m)}


def test_packed_wavefront_short_texts_end_at_their_own_length(answers):
    rs = answers["packed_unequal"]
    assert len({len(y) for _, y, *_ in rs}) == 1 and len(rs) <= 32  # one segment width, one wavefront
    for short, long_ in zip(rs[0::2], rs[1::2]):
        assert short[4] == len(short[0]) < len(long_[0]) and short[2] > 0  # its best end is its own |a|
        assert long_[1] == short[1] and long_[2] == 0 and long_[3] >= len(short[0])  # a perfect copy beyond the shorter text's length


def test_tile_edge_hits_start_and_end_at_the_edges(answers):
    rs = answers["tile_edges"]
    exact = {(start, end) for x, y, cost, start, end, _, _ in rs if cost == 0}
    assert {s for s, _ in exact} == set(cases.TILE_STARTS) and {e for _, e in exact} == set(cases.TILE_ENDS)
    R = cases.R
    long_ = [(start, end) for x, y, _, start, end, _, _ in rs if len(y) > 64 * R and len(x) == 200]
    assert {e for _, e in long_} >= {64, 128, 129}  # (their starts move: the inserted bytes find matches in the free flank)
    assert {len(y) for _, y, *_ in rs} >= {64 * R - 1, 64 * R, 64 * R + 1}

    def runs(cigar, op):
        return [k for k, o in ap.cigar_elems(cigar) if o == op]

    assert any(10 in runs(g, "D") and start == 20 for x, _, _, start, _, g, _ in rs if len(x) == 150)
    assert any(60 in runs(g, "I") for _, y, _, _, _, g, _ in rs if len(y) == 1160)
