"""The pairs of the ends-free diagonal-transition tests (tests/test_gpu_affine_dt_ends.py, tests/test_affine_dt_ends_plain.py), (a, b) =
(text, pattern), without a GPU in sight.  The ends-free lists and the global DT lists that bear on the mode are reused; three lists
stand at the kernel's own edges.  Under free_start front 0 is |a| + 1 diagonals wide where the bound is loose (the host leaves out the
diagonals above |a| - |b| + reach_ins(s_max), which no path within a tight bound can use), so a 64- or 256-diagonal round of it ends at
|a| = 63 or 255, and under free_end the found test is a minimum over the diagonals of every lane and wavefront of the block.

tied, lengths, tails and packed_unequal have a mean W of at most 256 and run in narrow blocks (one wavefront per pair) at every
bound.  Under free_start windows and long have a mean W above 256 and run in wide blocks (four wavefronts per pair) without a bound,
at the batch's largest cost and at that minus one; at s_max = 0 every list is narrow (tests/test_affine_dt_ends_plain.py computes
these widths by the host's rule)."""
from __future__ import annotations

import numpy as np

from tests.affine_dt_cases import lengths, tails
from tests.affine_ends_cases import MODELS, SETTING_MODELS, SETTINGS, any_byte, flanked, mutate, packed_unequal, planted, rand_seq  # noqa: F401


def tied(seed=21):
    """y * 8 against y, |y| = 40: tied ends at 40, 80, .. 320, in different lanes and (in a wide block) wavefronts, of which the lowest
    must win; the same with one byte inserted in the pattern (cost > 0); two planted copies; an empty pattern in a 300-byte text (end 0
    at s = 0); an empty text; |a| < |b|."""
    rng = np.random.default_rng(seed)
    y = rand_seq(rng, 40)
    z = rand_seq(rng, 60)
    two = rand_seq(rng, 35) + mutate(rng, z, 0.05) + rand_seq(rng, 50) + mutate(rng, z, 0.05) + rand_seq(rng, 20)
    return [
        (y * 8, y),
        (y * 8, y[:20] + (b"A" if y[20:21] != b"A" else b"C") + y[20:]),
        (two, z),
        (rand_seq(rng, 7) + z + rand_seq(rng, 90) + z + rand_seq(rng, 3), z),
        (rand_seq(rng, 300), b""),
        (b"", y),
        (b"", b""),
        (y[:17], y),
        (y[5:30], y),
    ]


WINDOW_TEXTS = (62, 63, 64, 65, 254, 255, 256, 257, 319, 320, 321)


def windows(seed=22):
    """8 x 150 bp in 400 bp at 5 %, and 100 bp patterns in texts of WINDOW_TEXTS bytes (front 0 ends on and next to a round of 64 or 256
    lanes; the shortest texts are windows of the mutated pattern).  Mean W > 256 under free_start: wide blocks."""
    rng = np.random.default_rng(seed)
    pairs = [planted(rng, 400, rand_seq(rng, 150), 0.05) for _ in range(8)]
    pairs += [planted(rng, n, rand_seq(rng, 100), 0.05) for n in WINDOW_TEXTS]
    return pairs


def long(seed=23):
    """One 2.1 kbp pattern in a 2.5 kbp window at 5 % next to one 60 bp read: many ring wraps, and mixed sizes in one launch."""
    rng = np.random.default_rng(seed)
    return [planted(rng, 2500, rand_seq(rng, 2100), 0.05), planted(rng, 140, rand_seq(rng, 60), 0.05)]


def all_cases():
    return dict(flanked=flanked(), packed_unequal=packed_unequal(), any_byte=any_byte(), lengths=lengths(), tails=tails(), tied=tied(),
                windows=windows(), long=long())
