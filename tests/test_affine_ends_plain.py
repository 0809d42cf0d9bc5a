"""The ends-free oracle (tests/affine_ends_plain.py) against tests/affine_plain.affine_nw: with both switches off it is affine_nw, and
with any of them on its cost is the least global cost over the substrings of the text that the switches allow."""
import numpy as np
import pytest

from tests import affine_plain as ap
from tests.affine_ends_cases import MODELS, SETTINGS, mutate, rand_seq
from tests.affine_ends_plain import affine_ends


def small_pairs(seed, count):
    """|a| <= 13, |b| <= 8 over two letters (ties are common), a third of them a mutated pattern between flanks."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(count):
        m = int(rng.integers(0, 9))
        y = rand_seq(rng, m, b"AC")
        if k % 3 == 0:
            core = mutate(rng, y, 0.2, b"AC")[:13]
            left = int(rng.integers(0, 13 - len(core) + 1))
            x = rand_seq(rng, left, b"AC") + core + rand_seq(rng, int(rng.integers(0, 13 - len(core) - left + 1)), b"AC")
        else:
            x = rand_seq(rng, int(rng.integers(0, 14)), b"AC")
        assert len(x) <= 13 and len(y) <= 8
        pairs.append((x, y))
    return pairs


@pytest.mark.parametrize("name", sorted(MODELS))
def test_both_switches_off_is_affine_nw(name):
    cm = MODELS[name]
    rng = np.random.default_rng(len(name))
    pairs = small_pairs(3, 30) + [(mutate(rng, y, 0.1), y) for y in (rand_seq(rng, m) for m in (40, 130, 300))]
    for x, y in pairs:
        cost, start, end, cigar, row = affine_ends(x, y, cm)
        assert (cost, cigar) == ap.affine_nw(x, y, cm)
        assert (start, end) == (0, len(x)) and row[-1] == cost and len(row) == len(x) + 1
        assert affine_ends(x, y, cm, trace=False)[0] == cost


@pytest.mark.parametrize("name", sorted(MODELS))
def test_cost_is_the_minimum_over_substrings(name):
    cm = MODELS[name]
    pairs = small_pairs(10 + len(name), 25)
    both_flanks = tied = 0
    for x, y in pairs:
        n = len(x)
        glob = {(s, e): ap.affine_nw(x[s:e], y, cm, trace=False)[0] for s in range(n + 1) for e in range(s, n + 1)}
        for fs, fe in SETTINGS:
            cost, start, end, cigar, row = affine_ends(x, y, cm, fs, fe)
            allowed = [(s, e) for (s, e) in glob if (fs or s == 0) and (fe or e == n)]
            assert cost == min(glob[se] for se in allowed), (x, y, fs, fe)
            # row[e] is the least cost over the allowed starts of the substrings that end at e
            assert row.tolist() == [min(glob[(s, e)] for s in range(e + 1) if fs or s == 0) for e in range(n + 1)]
            assert end == (int(np.flatnonzero(row == row.min())[0]) if fe else n) and row[end] == cost
            assert 0 <= start <= end and (fs or start == 0)
            assert ap.affine_verify(cigar, x[start:end], y, cm) == cost
            assert ap.no_adjacent_same_op(cigar)
            if fs and fe:
                both_flanks += 0 < start and end < n
                tied += int((row == row.min()).sum() > 1)
    assert both_flanks >= 1 and tied >= 1  # (the small cases reach what they are for)
