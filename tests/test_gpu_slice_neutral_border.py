"""The bit-sliced kernel (csrc/slice_kernel.hpp) runs the rows of EVERY lane in every step: a lane that has not reached column 0 is kept
in the left column's state by the neutral border value (hp, hm) = (0, ~0) instead of a predicate, a lane behind the last column computes
garbage that nothing may read, the boundary store's offset and the capture test's column are running counters.  This file aims at the
places where that can go wrong, at the smallest R the library offers (PA_SLICE=28: strips of 1792 rows), every distance against a plain DP
(tests/strip_plain.py):
  * columns n in {1, 2, 63, 64, 65, 127, 129}: fewer columns than lanes -- most lanes are outside most of the time, and a lane is in
    front of column 0 in one step and behind the end a few steps later -- or a last chunk of fewer than 64 steps;
  * rows m in {1, 1792, 1793, 3585}: one, two and three strips, so the boundary store and the poll run at n < 64 too;
  * a group whose 32 pairs have 32 different |a| from 1 on: an event in nearly every column, and the "no more events" value after the last;
  * a batch of 33 pairs, which ends in a group of one.
Every batch runs in reversed and in shuffled order and twice on its plan (tests/test_gpu_slice_edges.py: run_sliced)."""
import random

import numpy as np
import pytest

from tests import strip_plain
from tests.test_gpu_slice_edges import run_sliced
from tests.util_seq import mutate, rand_seq

pytestmark = pytest.mark.gpu

R = 28
STRIP = 64 * R
COLS = (1, 2, 63, 64, 65, 127, 129)
ROWS = (1, STRIP, STRIP + 1, 2 * STRIP + 1)


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


def plain_distance(a, b):
    s, _, _, _ = strip_plain.rect_dp(strip_plain.codes(a), strip_plain.codes(b), np.ones(len(a), np.int64), np.ones(len(b), np.int64))
    return s + len(b)  # D[m][n] = D[m][0] + sum, D[m][0] = m


def make_pair(n, m, seed):
    """|a| = n, |b| = m: unrelated, or b a mutated a (cut or padded to m: long diagonal runs)."""
    a = rand_seq(n, seed, 1)
    if seed % 3 == 0:
        return a, rand_seq(m, seed, 2)
    b = mutate(a, (0.03, 0.2)[seed % 2], seed)
    b = b[:m] if len(b) >= m else b + rand_seq(m - len(b), seed, 5)
    return a, b


def group(n, m, seed, a_lens=None):
    """32 pairs, the widest n columns and the tallest m rows; several pairs reach the last row of the last strip or end just short of it."""
    rng = random.Random(seed)
    ns = a_lens or [n] + [rng.randint(1, n) for _ in range(31)]
    ms = [m, m, max(1, m - 1), max(1, m - STRIP), max(1, m - STRIP + 1)] + [rng.randint(1, m) for _ in range(27)]
    pairs = [make_pair(x, y, seed * 100 + i) for i, (x, y) in enumerate(zip(ns, ms))]
    return pairs, [plain_distance(a, b) for a, b in pairs]


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", COLS)
def test_columns_by_strips(pa, monkeypatch, n, m):
    pairs, want = cached((n, m), lambda: group(n, m, seed=1000 * n + m))
    assert max(len(a) for a, _ in pairs) == n and max(len(b) for _, b in pairs) == m
    run_sliced(pa, monkeypatch, R, pairs, want, distinct=False)


@pytest.mark.parametrize("m", ROWS)
def test_event_in_every_column(pa, monkeypatch, m):
    """|a| = 1 .. 32: 32 capture events in consecutive columns from column 1 on, the last one followed by the value that means "none"."""
    pairs, want = cached(("events", m), lambda: group(32, m, seed=77 + m, a_lens=list(range(1, 33))))
    assert sorted(len(a) for a, _ in pairs) == list(range(1, 33))
    run_sliced(pa, monkeypatch, R, pairs, want, distinct=False)


@pytest.mark.parametrize("m", (STRIP, STRIP + 1))
def test_group_of_one(pa, monkeypatch, m):
    """33 pairs: the widest is alone in the last group (one capture event, one live bit), in one strip and in two."""
    def make():
        pairs, want = group(63, m, seed=5 + m)
        a, b = make_pair(65, m, 4242)
        return pairs + [(a, b)], want + [plain_distance(a, b)]

    pairs, want = cached(("one", m), make)
    assert len(pairs) == 33
    run_sliced(pa, monkeypatch, R, pairs, want, distinct=False)
