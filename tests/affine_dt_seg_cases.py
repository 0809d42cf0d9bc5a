"""The pairs at which only the segmented traceback of the diagonal-transition route can go wrong (tests/test_affine_dt_seg_plain.py,
tests/test_gpu_affine_dt_seg.py), without a GPU in sight.  The route cuts the costs into segments of `seg` costs and hands the walk from
one segment to the next through a stored state, so what matters is where the cost and the walk stand against the segment boundaries:
a gap that is open across several boundaries (the walk crosses them inside the insert or delete layer), costs of 0, below the largest
edge, on and next to a multiple of seg, and a cost of many segments at the default seg."""
from __future__ import annotations

import numpy as np

from tests.affine_ends_cases import MODELS, mutate, rand_seq  # noqa: F401

GAP = 40
GAP_MODELS = ("affine", "linear_affine", "affine_asymmetric")  # the models under which a 40-byte gap runs on an affine layer


def gaps(seed=31):
    """A deletion and an insertion of GAP bytes between two matching flanks of 50 and 45 bytes (a has the bytes b lacks: a deletion;
    then the same pair swapped).  The gap's bytes are of another alphabet than the flanks, so that the one long gap is the only
    optimal path.  Under affine(4, 6, 2) it costs 86, and at seg = 8 the walk stays in the layer across ten boundaries."""
    rng = np.random.default_rng(seed)
    left, right, mid = rand_seq(rng, 50), rand_seq(rng, 45), rand_seq(rng, GAP, b"NRYK")
    a, b = left + mid + right, left + right
    return [(a, b), (b, a)]


def small(seed=32):
    """Equal sequences (cost 0, one segment, no fill but that of front 0), and pairs whose cost is below the largest edge of most
    models: one substitution, one inserted byte, one deleted byte; and two and three substitutions, which put the cost on and next to
    small multiples."""
    rng = np.random.default_rng(seed)
    x = rand_seq(rng, 70)
    flip = lambda c: b"A" if c != b"A" else b"C"  # noqa: E731
    sub1 = x[:30] + flip(x[30:31]) + x[31:]
    sub2 = sub1[:50] + flip(sub1[50:51]) + sub1[51:]
    sub3 = sub2[:10] + flip(sub2[10:11]) + sub2[11:]
    return [(x, x), (x, sub1), (x, x[:40] + b"N" + x[40:]), (x, x[:20] + x[21:]), (x, sub2), (x, sub3), (b"", b""), (x[:9], b"")]


def ladder(seed=33):
    """One 60-byte sequence against itself with 1 .. 12 substitutions: costs sub, 2 sub, .. 12 sub under every model, so that every
    residue of the cost modulo a small seg occurs, 0, 1 and seg - 1 among them."""
    rng = np.random.default_rng(seed)
    x = rand_seq(rng, 60, b"AC")
    pairs, y = [], bytearray(x)
    for q in range(12):
        y[3 + 5 * q - (q % 2)] = ord("G")
        pairs.append((x, bytes(y)))
    return pairs


def many(seed=34):
    """One pair of about 2 kbp at 10 %: dozens of segments at the default seg, hundreds at seg = E."""
    rng = np.random.default_rng(seed)
    x = rand_seq(rng, 2000)
    return [(x, mutate(rng, x, 0.10))]


def all_cases():
    return dict(gaps=gaps(), small=small(), ladder=ladder(), many=many())
