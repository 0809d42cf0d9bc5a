"""The bit-sliced kernel with an ODD number of rows per lane (csrc/slice_kernel.hpp: pair blocks, then PA_SLICE_ROW_ONE for the last row)
and on boundary rows that only the kernel itself has reset (the strips hand the columns they consumed back as "not written";
slice_unit.hip clears the buffer when the plan is created and after a pass that did not finish).

PA_SLICE = 45, 49, 51.  |b| at the strip edges of that R -- 1, 64 R - 1, 64 R, 64 R + 1, 128 R, 128 R + 1 (one, two and three strips) --
against |a| at the chunk edges 1, 63, 64, 65, 130: one ragged group of 32 pairs and a batch of 70 (three groups, the last one of six).
Every distance against oracle.levenshtein; each batch runs three times on its resident plan: the second and the third pass find the
boundary rows as the first one's consumers left them."""
import numpy as np
import pytest

from tests.util_seq import mutate, rand_seq

pytestmark = pytest.mark.gpu

ODD_ROWS = (45, 49, 51)
A_LENS = (1, 63, 64, 65, 130)


def b_lens(R):
    s = 64 * R
    return (1, s - 1, s, s + 1, 2 * s, 2 * s + 1)


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


_cache = {}


def batch_for(R, count, oracle):
    """`count` pairs over the 30 combinations of (|a|, |b|) in turn; b starts as a mutated copy of a where it is long enough to hold one
    and goes on at random, so the distance depends on the rows of every strip's top.  -> (pairs, distances), made once per (R, count)."""
    key = (R, count)
    if key not in _cache:
        combos = [(n, m) for m in b_lens(R) for n in A_LENS]
        pairs = []
        for i in range(count):
            n, m = combos[(7 * i) % len(combos)]
            a = rand_seq(n, 1000 * R + i, 1)
            head = mutate(a, (0.02, 0.1, 0.3)[i % 3], 1000 * R + i)[:m]
            b = head + rand_seq(m - len(head), 1000 * R + i, 2)
            assert len(a) == n and len(b) == m
            pairs.append((a, b))
        _cache[key] = (pairs, [oracle.levenshtein(a, b) for a, b in pairs])
    return _cache[key]


@pytest.mark.parametrize("count", [32, 70])
@pytest.mark.parametrize("R", ODD_ROWS)
def test_odd_rows_three_passes(pa, oracle, monkeypatch, R, count):
    pairs, want = batch_for(R, count, oracle)
    assert {len(b) for _, b in pairs} == set(b_lens(R)) and {len(a) for a, _ in pairs} == set(A_LENS)
    monkeypatch.setenv("PA_SLICE", str(R))
    bt = pa.Batch(pairs)
    try:
        sh = bt.shape()
        assert sh["kernel"].startswith("pa::slice::slice_kernel<") and sh["sliced_rows_per_lane"] == R, sh
        assert sh["groups"] == -(-count // 32) and sh["boundary_bytes"] > 0, sh
        passes = [bt.run()[0].copy() for _ in range(3)]
    finally:
        bt.close()
    bad = [i for i, (c, w) in enumerate(zip(passes[0].tolist(), want)) if c != w]
    assert not bad, ", ".join(f"#{i} |a|={len(pairs[i][0])} |b|={len(pairs[i][1])}: {int(passes[0][i])} != {want[i]}" for i in bad[:8])
    assert np.array_equal(passes[0], passes[1]) and np.array_equal(passes[0], passes[2])
