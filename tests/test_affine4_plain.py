"""The double-affine oracles of tests/affine4_plain.py against each other, against known answers and, with layers 2 and 3 priced out,
against the two-layer oracle of tests/affine_plain.py (CPU only)."""
import numpy as np
import pytest

from astar_pairwise_aligner_amd import AffineCost
from tests import affine4_plain as a4
from tests import affine_plain as ap

DOUBLE = AffineCost.double_affine(4, 6, 2, 24, 1)
MODELS = {
    "double_affine": DOUBLE,
    "linear_edges": AffineCost(3, 5, 4, [("ins", 4, 2), ("del", 3, 2), ("ins", 12, 1), ("del", 14, 1)]),
    "no_sub": AffineCost(None, None, None, [("ins", 2, 2), ("del", 2, 2), ("ins", 9, 1), ("del", 9, 1)]),
    "asymmetric": AffineCost(5, None, None, [("ins", 3, 3), ("del", 7, 2), ("ins", 15, 1), ("del", 20, 1)]),
}


def cut2(cm):
    """The same model cut to its first two layers."""
    return AffineCost(cm.sub, cm.ins, cm.del_, cm.layers[:2])


def seeded_pairs(seed, count, max_len=45, max_gap=30):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(count):
        n = int(rng.integers(0, max_len + 1))
        x = bytes(b"ACGT"[k] for k in rng.integers(0, 4, n))
        y = bytearray(x)
        for _ in range(int(rng.integers(0, 3))):  # up to two long gaps, either way
            L = int(rng.integers(1, max_gap + 1))
            at = int(rng.integers(0, len(y) + 1))
            if rng.random() < 0.5:
                y[at:at] = bytes(b"ACGT"[k] for k in rng.integers(0, 4, L))
            else:
                del y[at:at + L]
        for _ in range(int(rng.integers(0, 4))):
            if y:
                y[int(rng.integers(0, len(y)))] = b"ACGT"[int(rng.integers(0, 4))]
        pairs.append((x, bytes(y[:max_len])))
    return pairs


@pytest.mark.parametrize("name", sorted(MODELS))
def test_layered_equals_general_gap(name):
    cm = MODELS[name]
    differ = 0
    for x, y in seeded_pairs(len(name), 100):
        c, g = a4.affine4_nw(x, y, cm)
        assert c == a4.general_gap_cost(x, y, cm), (x, y)
        assert a4.affine4_verify(g, x, y, cm) == c, (x, y, g)
        assert ap.no_adjacent_same_op(g), g
        assert a4.affine4_nw(x, y, cm, trace=False)[0] == c
        differ += ap.affine_nw(x, y, cut2(cm), trace=False)[0] != c
    assert differ > 0, "layers 2 and 3 never mattered"


def test_known_answers():
    x, y = b"A" * 30 + b"C" * 40 + b"G" * 30, b"A" * 30 + b"G" * 30
    assert a4.affine4_nw(x, y, DOUBLE)[0] == 64
    assert ap.affine_nw(x, y, AffineCost.affine(4, 6, 2))[0] == 86
    for L, want in ((18, 42), (19, 43)):  # the pieces cross at 18: 6 + 2 L = 24 + L
        x, y = b"ACGT" * 5 + b"T" * L + b"GATC" * 5, b"ACGT" * 5 + b"GATC" * 5
        c, g = a4.affine4_nw(x, y, DOUBLE)
        assert c == want and a4.affine4_verify(g, x, y, DOUBLE) == want
        c, g = a4.affine4_nw(y, x, DOUBLE)
        assert c == want and a4.affine4_verify(g, y, x, DOUBLE) == want
    assert a4.gap_cost(18, None, [(6, 2), (24, 1)]) == 42 and a4.gap_cost(19, None, [(6, 2), (24, 1)]) == 43


@pytest.mark.parametrize("two", [AffineCost.affine(4, 6, 2), AffineCost.linear_affine(3, 2, 4, 1), AffineCost.affine_asymmetric(5, 3, 1, 7, 2),
                                 AffineCost(None, 2, None, [("ins", 3, 1), ("del", 2, 2)])])
def test_reduction_to_two_layers(two):
    """Layers 2 and 3 at open = 1000 with layer 0 and 1's extends are strictly worse in every cell, and the close of layer 0 / 1 precedes
    theirs in parent order: cost AND CIGAR are the two-layer oracle's."""
    (_, _, e0), (_, _, e1) = two.layers
    four = AffineCost(two.sub, two.ins, two.del_, two.layers + [("ins", 1000, e0), ("del", 1000, e1)])
    pairs = seeded_pairs(99, 60, max_len=70) + [(b"", b""), (b"", b"ACG"), (b"ACG", b""), (b"A" * 200, b"A" * 150 + b"C" * 3)]
    for x, y in pairs:
        assert a4.affine4_nw(x, y, four) == ap.affine_nw(x, y, two), (x, y)


def test_other_layer_lists_are_refused():
    for cm in (AffineCost.affine(4, 6, 2), AffineCost.unit(), AffineCost(1, None, None, [("del", 1, 1), ("ins", 1, 1), ("ins", 2, 1), ("del", 2, 1)])):
        with pytest.raises(ValueError):
            a4.affine4_nw(b"A", b"A", cm)
        with pytest.raises(ValueError):
            a4.general_gap_cost(b"A", b"A", cm)
