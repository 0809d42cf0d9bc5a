"""The pairs of the diagonal-transition tests (tests/test_gpu_affine_dt.py, tests/test_affine_dt_plain.py), without a GPU in sight: the
smallest shapes at which the DT kernel can go wrong.  Lanes own diagonals 64 at a time, the extension compares 8 bytes per load, and the
ring of fronts wraps every `largest edge + 1` cost steps; the lists below put lengths, match runs, front widths and end diagonals on and
around those numbers."""
from __future__ import annotations

import numpy as np

from tests.affine_ends_cases import MODELS, mutate, rand_seq  # noqa: F401  (the seven constructors, at the costs of the ends-free tests)

LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def lengths(seed=11):
    """Every |a| x |b| of LENGTHS (both empty and one empty among them): unrelated, related and equal-prefix pairs in turn."""
    rng = np.random.default_rng(seed)
    pairs = []
    for x, n in enumerate(LENGTHS):
        for y, m in enumerate(LENGTHS):
            a = rand_seq(rng, n)
            kind = (x + y) % 3
            if kind == 0:
                b = rand_seq(rng, m)
            elif kind == 1:
                b = (mutate(rng, a, 0.2) + rand_seq(rng, m))[:m]
            else:
                b = (a + rand_seq(rng, m))[:m]  # one is a prefix of the other: a match run to a sequence end, then one gap
            pairs.append((a, b))
    return pairs


def tails(seed=12):
    """Equal sequences, sequences that differ only in the last or only in the first byte, and match runs that end exactly at a sequence
    end and exactly at a 4- and 8-byte boundary of either sequence (the extension's tail)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for n in (1, 4, 7, 8, 9, 16, 23, 24, 25, 64, 100):
        a = rand_seq(rng, n)
        flip = lambda c: b"A" if c != b"A" else b"C"  # noqa: E731
        pairs.append((a, a))
        pairs.append((a, a[:-1] + flip(a[-1:])))
        pairs.append((a, flip(a[:1]) + a[1:]))
    base = rand_seq(rng, 40, b"AC")
    for run in (3, 4, 5, 7, 8, 9, 12, 15, 16, 17):
        for shift in (0, 1, 3, 4):  # b starts `shift` bytes later in its buffer's terms: the run ends at another alignment of b
            a = base[:run] + b"G" + base[run:]
            b = rand_seq(rng, shift, b"T") + base[:run] + b"T" + base[run:]
            pairs.append((a, b))
            pairs.append((a[:run], b))          # the run ends at the end of a
            pairs.append((a, b[:shift + run]))  # ... at the end of b
    return pairs


def wide(seed=13):
    """Unrelated random pairs of 80 .. 200 bp: the front grows past 64 and past 128 diagonals, and the ring wraps many times."""
    rng = np.random.default_rng(seed)
    return [(rand_seq(rng, int(rng.integers(80, 201))), rand_seq(rng, int(rng.integers(80, 201)))) for _ in range(10)]


def far_diagonals(seed=14):
    """|a| - |b| = +-70 and +-130: the end diagonal lies outside the first group of 64 lanes, on either side."""
    rng = np.random.default_rng(seed)
    pairs = []
    for gap in (70, 130):
        core = rand_seq(rng, 90)
        left, right = int(rng.integers(0, gap + 1)), 0
        right = gap - left
        long_ = rand_seq(rng, left) + mutate(rng, core, 0.05) + rand_seq(rng, right)
        long_ = long_[:len(core) + gap] + rand_seq(rng, max(0, len(core) + gap - len(long_)))
        assert len(long_) - len(core) == gap
        pairs += [(long_, core), (core, long_)]
    return pairs


def low_complexity(seed=15):
    """Every diagonal extends far and ties are many: runs of one letter of two lengths, short tandem repeats."""
    rng = np.random.default_rng(seed)
    pairs = [(b"A" * n, b"A" * m) for n, m in ((5, 9), (33, 30), (64, 71), (100, 65), (17, 0))]
    for unit, ca, cb in ((b"AC", 20, 26), (b"ACG", 21, 17), (b"AAC", 30, 33), (b"ACGT", 16, 19)):
        pairs.append((unit * ca, unit * cb))
        pairs.append((unit * ca + b"T" + unit * 3, unit * 2 + b"G" + unit * cb))
    pairs.append((mutate(rng, b"AC" * 60, 0.05), mutate(rng, b"AC" * 60, 0.05)))
    return pairs


def mixed(seed=16):
    """Reads with two pairs of 2 .. 3 kbp at about 10 %: long and short pairs in one launch, many cost steps, fronts a few hundred wide."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(12):
        x = rand_seq(rng, int(rng.integers(100, 200)))
        pairs.append((x, mutate(rng, x, 0.08)))
    for n in (2100, 2900):
        x = rand_seq(rng, n)
        pairs.insert(3 if n == 2100 else 9, (x, mutate(rng, x, 0.10)))
    return pairs


def all_cases():
    return dict(lengths=lengths(), tails=tails(), wide=wide(), far_diagonals=far_diagonals(), low_complexity=low_complexity(), mixed=mixed())
