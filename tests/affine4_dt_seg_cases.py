"""The pairs and the model that only the segmented traceback of the double-affine diagonal-transition route needs
(tests/test_affine4_dt_seg_plain.py, tests/test_gpu_affine4_dt_seg.py), without a GPU in sight.  The lists of tests/affine4_dt_cases.py
and of tests/affine_dt_seg_cases.py (small, ladder, many) are reused as they are; what they lack is

  long_gap  a gap of LONG_GAP = 100 foreign bytes between matching flanks, as a deletion and as an insertion.  Under
            double_affine(4, 6, 2, 24, 1) it costs 124 on the second piece, and at seg = 24 the walk crosses four boundaries inside
            layer 4 (deletion) or layer 3 (insertion) and then one on the main layer.  The 18-byte gaps of affine4_dt_cases.gaps() (cost
            42 on the first piece) cross one boundary inside layers 2 and 1.
  STEEP     a model whose extends (9, 9, 8, 8) cost more than every open (1, 1, 2, 2) and than the substitution (2): E = 2 but
            Ew = 9, so a segment may be no shorter than 9 although the main layer is never read further back than 2.  A gap of 18
            bytes costs 2 + 18 x 8 = 146 and crosses sixteen boundaries inside its layer at seg = 9.
"""
from __future__ import annotations

import numpy as np

from astar_pairwise_aligner_amd import AffineCost
from tests import affine4_dt_cases as dt4_cases
from tests import affine_dt_seg_cases as seg_cases
from tests.affine4_ends_cases import MODELS as BASE_MODELS
from tests.affine4_ends_cases import OTHER
from tests.affine_ends_cases import SETTINGS, rand_seq  # noqa: F401

STEEP = AffineCost(2, None, None, [("ins", 1, 9), ("del", 1, 9), ("ins", 2, 8), ("del", 2, 8)])
MODELS = dict(BASE_MODELS, steep=STEEP)
LONG_GAP = 100


def long_gap(seed=61):
    rng = np.random.default_rng(seed)
    left, right, mid = rand_seq(rng, 50), rand_seq(rng, 45), rand_seq(rng, LONG_GAP, OTHER)
    a, b = left + mid + right, left + right
    return [(a, b), (b, a)]


def gap18():
    """The pairs of affine4_dt_cases.gaps() whose gap is 18 bytes inside the pair: a deletion, then an insertion."""
    at = 6 * dt4_cases.GAP_LENGTHS.index(18)
    return dt4_cases.gaps()[at:at + 2]


def new_cases():
    """What this route's tests add to the lists of the DT tests."""
    return dict(long_gap=long_gap(), small=seg_cases.small(), ladder=seg_cases.ladder())


def many():
    return seg_cases.many()
