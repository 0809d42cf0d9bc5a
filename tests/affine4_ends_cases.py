"""The pairs of the double-affine ends-free tests (tests/test_gpu_affine4_ends.py), (a, b) = (text, pattern).  The shapes are those of
tests/affine_ends_cases.py, whose generators are reused as they are (both batches have 16 rows per lane); two_piece() adds what only two
gap pieces can get wrong.  tests/test_affine4_ends_cases.py asks the plain DP, without a GPU, whether the pairs are worth running."""
from __future__ import annotations

import numpy as np

from astar_pairwise_aligner_amd import AffineCost
from tests.affine_ends_cases import (EDGE_M, R, SETTINGS, TILE_COLS, any_byte, edge_all, edge_pairs, flanked, packed_unequal,  # noqa: F401
                                     rand_seq, tile_edges)

DOUBLE = AffineCost.double_affine(4, 6, 2, 24, 1)  # a gap of length L costs min(6 + 2 L, 24 + L): the second piece wins from L = 19
ASYMMETRIC = AffineCost(5, None, None, [("ins", 3, 3), ("del", 7, 2), ("ins", 15, 1), ("del", 20, 1)])
LINEAR_EDGES = AffineCost(3, 5, 4, [("ins", 4, 2), ("del", 3, 2), ("ins", 12, 1), ("del", 14, 1)])
MODELS = {"double_affine": DOUBLE, "asymmetric": ASYMMETRIC, "linear_edges": LINEAR_EDGES}
SECOND_PIECE_FROM = 19

OTHER = b"KLMN"  # bytes no text or pattern of ACGT holds: a run of them can only be a gap or substitutions


def two_piece(seed=9):
    """Under DOUBLE, with both ends free, in this order:
      0  a deletion run of 30 columns that crosses column 64 (text x, pattern x[20:55] + x[85:120]);
      1  an insertion run of 40 rows that crosses row 64 R;
      2  an insertion run of 40 rows that is the pattern's first 40 rows: the walk reaches row 0 out of layer 2;
      3  a hit whose best end comes 24 columns after a deletion run of 20: a wrong D2 would move the end."""
    rng = np.random.default_rng(seed)
    pairs = []
    x = rand_seq(rng, 150)
    pairs.append((x, x[20:55] + x[85:120]))
    y = rand_seq(rng, 64 * R + 100)
    pairs.append((rand_seq(rng, 30) + y + rand_seq(rng, 30), y[:64 * R - 24] + rand_seq(rng, 40, OTHER) + y[64 * R - 24:]))
    y = rand_seq(rng, 100)
    pairs.append((rand_seq(rng, 45) + y + rand_seq(rng, 20), rand_seq(rng, 40, OTHER) + y))
    x = rand_seq(rng, 30) + (y := rand_seq(rng, 50)) + rand_seq(rng, 20, OTHER) + (z := rand_seq(rng, 24)) + rand_seq(rng, 40)
    pairs.append((x, y + z))
    return pairs
