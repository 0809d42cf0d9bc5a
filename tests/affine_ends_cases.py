"""The pairs of the ends-free tests (tests/test_gpu_affine_ends.py), (a, b) = (text, pattern), and the settings they run under.  They live
here, without a GPU in sight, so that tests/test_affine_ends_cases.py can ask the plain DP whether they are worth running: hits away from
both ends of the text, tied minima in the last row, ends at column 0 and at |a|, texts shorter than the pattern and empty ones."""
from __future__ import annotations

import numpy as np

from astar_pairwise_aligner_amd import AffineCost
from astar_pairwise_aligner_amd.capi import AFFINE_ROWS_PER_LANE as R

MODELS = {
    "lcs": AffineCost.lcs(),
    "unit": AffineCost.unit(),
    "linear": AffineCost.linear(3, 2),
    "linear_asymmetric": AffineCost.linear_asymmetric(2, 1, 3),
    "affine": AffineCost.affine(4, 6, 2),
    "linear_affine": AffineCost.linear_affine(3, 2, 4, 1),
    "affine_asymmetric": AffineCost.affine_asymmetric(5, 3, 1, 7, 2),
}
SETTINGS = ((False, False), (True, False), (False, True), (True, True))  # (free_start, free_end)
SETTING_MODELS = ("affine", "linear_affine", "lcs")                      # the models every setting runs under

# |b|: one lane, several lanes, a full segment, two and three strips
EDGE_M = (0, 1, R, R + 1, 4 * R + 3, 64 * R - 1, 64 * R, 64 * R + 1, 128 * R + 77)


def edge_n(m):
    return (0, m // 2, m, m + 37, 2 * m + 5)


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def mutate(rng, s: bytes, rate: float, alphabet=b"ACGT") -> bytes:
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(alphabet[rng.integers(0, len(alphabet))])
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out += bytes([ch, alphabet[rng.integers(0, len(alphabet))]])
        else:
            out.append(ch)
    return bytes(out)


def planted(rng, n, b, rate=0.1, alphabet=b"ACGT"):
    """The usual pair: a text of n bytes, random flank + mutate(b) + random flank; a window of mutate(b) where that is longer than n."""
    core = mutate(rng, b, rate, alphabet)
    if len(core) > n:
        off = int(rng.integers(0, len(core) - n + 1))
        return core[off:off + n], b
    left = int(rng.integers(0, n - len(core) + 1))
    return rand_seq(rng, left, alphabet) + core + rand_seq(rng, n - len(core) - left, alphabet), b


def edge_pairs(rot):
    """One pair per |b| of EDGE_M: |a| = edge_n(|b|)[(k + rot) % 5] for the k-th |b|."""
    rng = np.random.default_rng(100 + rot)
    return [planted(rng, edge_n(m)[(k + rot) % 5], rand_seq(rng, m)) for k, m in enumerate(EDGE_M)]


def edge_all():
    """Every |b| of EDGE_M with every |a| of edge_n(|b|): the five rotations of edge_pairs."""
    return [p for rot in range(5) for p in edge_pairs(rot)]


def flanked(seed=1, count=24):
    """Small usual pairs, then the special ones: a tied last-row minimum (a = b + b), an end at column 0 (an empty pattern; a pattern
    unrelated to a tiny text), an end at |a| (the hit is the text's suffix), |a| < |b| and |a| = 0."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(count):
        m = int(rng.integers(5, 300))
        pairs.append(planted(rng, m + int(rng.integers(8, 120)), rand_seq(rng, m), 0.08))
    y = rand_seq(rng, 40)
    pairs += [(y + y, y), (rand_seq(rng, 30), b""), (b"AC", b"GGGGGGGG"), (rand_seq(rng, 25) + y, y), (y[:17], y), (b"", y), (b"", b"")]
    return pairs


def packed_unequal(seed=2):
    """Pairs of one segment width (|b| = 24: two lanes, 32 pairs to a wavefront) whose texts differ in length.  Every even pair's hit is
    the suffix of its text, so its best end is its own |a|; the odd pair after it shares the pattern, and its longer text goes on with a
    perfect copy of the pattern beyond the shorter one's length: a pair that looked past its own |a| into its wavefront's longer
    columns would be wrong, not lucky."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(12):
        y = rand_seq(rng, 24)
        short = rand_seq(rng, 5 + 3 * k) + y[:11] + y[12:]  # the hit lacks one byte of the pattern: its cost is not zero
        pairs.append((short, y))
        pairs.append((rand_seq(rng, len(short) + 2) + y + rand_seq(rng, 7), y))
    return pairs


TILE_COLS = 64
TILE_STARTS, TILE_ENDS = (0, 63, 64, 65), (64, 65, 128, 129)


def tile_edges(seed=3):
    """For align_tiled(64): exact hits a[start:end] with start and end on and next to the column-tile edges, the same hits with 1000
    pattern bytes inserted in their middle (|b| > 64 R: the walk crosses the row-tile edge, in an insertion run), |b| = 64 R - 1, 64 R and
    64 R + 1 at a diagonal, and gaps that are open across a tile edge: a deletion run over columns 60 .. 70, an insertion run over rows
    1000 .. 1060."""
    rng = np.random.default_rng(seed)
    pairs = []
    for st in TILE_STARTS:
        for en in TILE_ENDS:
            if en - st < 24:
                continue
            x = rand_seq(rng, 200)
            hit = x[st:en]
            pairs.append((x, hit))
            if (st, en) in ((0, 64), (63, 128), (64, 129), (65, 129)):
                pairs.append((x, hit[:12] + rand_seq(rng, 1000) + hit[12:]))
    for m in (64 * R - 1, 64 * R, 64 * R + 1):
        pairs.append(planted(rng, m + 70, rand_seq(rng, m), 0.05))
    x = rand_seq(rng, 150)
    pairs.append((x, x[20:60] + x[70:110]))  # D over columns 61 .. 70
    y = rand_seq(rng, 1100)
    pairs.append((rand_seq(rng, 30) + y + rand_seq(rng, 30), y[:1000] + rand_seq(rng, 60) + y[1000:]))  # I over rows 1001 .. 1060
    return pairs


def any_byte(seed=6):
    """tests/test_gpu_affine.test_any_byte's alphabets, with flanks: protein letters and every byte value."""
    rng = np.random.default_rng(seed)
    protein = b"ACDEFGHIKLMNPQRSTVWY"
    every = bytes(range(256))
    pairs = []
    for k in range(6):
        y = rand_seq(rng, 40 + 90 * k, protein)
        pairs.append(planted(rng, len(y) + 50, y, 0.15, protein))
    y = bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    pairs.append(planted(rng, 640, y, 0.1, every))
    pairs.append((b"\x00\xff" * 40, b"\xff\x00" * 21))
    pairs.append((b"acgtnNACGT" * 20, b"ACGTNnacgt" * 9))
    return pairs


def all_cases(rots=range(5)):
    """Every generator's pairs, by name; of the edge shapes the rotations `rots`."""
    d = {f"edge{rot}": edge_pairs(rot) for rot in rots}
    d.update(flanked=flanked(), packed_unequal=packed_unequal(), tile_edges=tile_edges(), any_byte=any_byte())
    return d
