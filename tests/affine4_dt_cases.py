"""The pairs of the double-affine diagonal-transition tests (tests/test_gpu_affine4_dt.py, tests/test_affine4_dt_plain.py), without a GPU
in sight: the lists of tests/affine_dt_cases.py and tests/affine_dt_ends_cases.py reused as they are, plus what four layers add.

  gaps        one gap of every length of GAP_LENGTHS, as an insertion and as a deletion, inside the pair, at its start and at its end.
              The lengths stand on and around the crossovers of the three models of affine4_ends_cases.MODELS: 6 + 2 L against 24 + L
              (equal at 18, the second piece wins from SECOND_PIECE_FROM = 19), ASYMMETRIC's 3 + 3 L against 15 + L (6 | 7) and
              7 + 2 L against 20 + L (13 | 14), LINEAR_EDGES' 5 L against 4 + 2 L (1 | 2), 4 + 2 L against 12 + L (8 | 9), 4 L against
              3 + 2 L (1 | 2) and 3 + 2 L against 14 + L (11 | 12); and 40, far inside the second piece.
  ring_wraps  unrelated pairs of 60 .. 90 bp: the cost is several wraps of the deepest ring (25 slots of the main layer under DOUBLE) and
              many of the shallowest (2 slots of a layer with extend 1).
  mixed       affine_dt_cases.mixed: reads next to two pairs of 2 .. 3 kbp at 10 %.  Its mean W at the bound is above 256, so its blocks
              are wide (four wavefronts per pair), as are wide and far_diagonals; lengths, tails, low_complexity, gaps and ring_wraps stay
              below and run in narrow blocks.
"""
from __future__ import annotations

import numpy as np

from tests import affine_dt_cases as dt_cases
from tests import affine_dt_ends_cases as ends_cases
from tests.affine4_ends_cases import ASYMMETRIC, DOUBLE, LINEAR_EDGES, MODELS, OTHER, SECOND_PIECE_FROM, two_piece  # noqa: F401
from tests.affine_ends_cases import SETTINGS, rand_seq  # noqa: F401

GAP_LENGTHS = (1, 2, 3, 6, 7, 8, 9, 11, 12, 13, 14, 17, 18, 19, 20, 40)
WIDE_MEAN = 256  # affine4_dt_plan.hpp's kWideMean


def gaps(seed=31):
    """For every L of GAP_LENGTHS: (x with L foreign bytes, x) and (x, x with L foreign bytes), the run inside x, before it and after
    it.  The foreign bytes match nothing, so the cheapest path pays one gap of exactly L."""
    rng = np.random.default_rng(seed)
    pairs = []
    for L in GAP_LENGTHS:
        x = rand_seq(rng, 70)
        g = rand_seq(rng, L, OTHER)
        for y in (x[:33] + g + x[33:], g + x, x + g):
            pairs += [(y, x), (x, y)]
    return pairs


def ring_wraps(seed=32):
    rng = np.random.default_rng(seed)
    return [(rand_seq(rng, int(rng.integers(60, 91))), rand_seq(rng, int(rng.integers(60, 91)))) for _ in range(6)]


def global_cases():
    """The lists of the global calls (run_dt, align_dt)."""
    return dict(dt_cases.all_cases(), gaps=gaps(), ring_wraps=ring_wraps())


def ends_gaps(seed=33):
    """gaps() as patterns in a window: every pair of gaps() with 25 + 30 bytes of text around a."""
    rng = np.random.default_rng(seed)
    return [(rand_seq(rng, 25) + a + rand_seq(rng, 30), b) for a, b in gaps()[::2]] + gaps()[1::2]


def ends_cases_all():
    """The lists of the ends-free calls (run_dt_ends, align_dt_ends)."""
    return dict(ends_cases.all_cases(), gaps=ends_gaps(), two_piece=two_piece())


# the 2 .. 3 kbp lists run under one model: the numpy oracle takes seconds a pair there
LONG_LISTS = {"mixed": "double_affine", "long": "double_affine"}


def models_of(case: str):
    return [LONG_LISTS[case]] if case in LONG_LISTS else sorted(MODELS)
