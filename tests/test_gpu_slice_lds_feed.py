"""The bit-sliced kernel's column ring (csrc/slice_kernel.hpp, "The column ring"): a column's code planes and the boundary row's (hp, hm) are
written into LDS once per chunk of 64 columns and read from there by every lane, every step; lane 0 takes the row above from the ring,
every other lane from the lane above it.

What can go wrong there sits at the chunk edges (the write at the chunk top, the read of the chunk's first step behind it), at the ring's
wrap (256 entries), in the last chunk (no prefetch) and in what lane 0 takes in: the matrix's top border in a strip without a strip above,
polled boundary data below one, and both in a middle strip.  So: PA_SLICE = 28 (strips of 1792 rows), groups whose longest a is
1, 63, 64, 65, 128, 129, 255, 256, 257 and 513 columns, each with one, two and three strips; the |a| of a group differ where its range allows (capture
events in the middle of a chunk and at a chunk edge), so do the |b|; one batch ends in a group of 6 pairs.  Every batch runs twice on its
plan (the boundary rows reset themselves), and twice more with PA_SLICE_GRID=1, where the jobs run strictly in ticket order, a consumer
after its producer has finished.  Every distance against oracle.nw_cost and against the strip kernels (PA_SLICE=0)."""
import numpy as np
import pytest

from tests.util_seq import mutate, rand_seq

pytestmark = pytest.mark.gpu

R = 28
STRIP = 64 * R
# (the longest a of the batch's groups, pairs in the batch): groups are cut by |a|, 32 pairs each, the last one takes the rest
BATCHES = {"1-63-64": ((1, 63, 64), 96), "65-128-129": ((65, 128, 129), 96), "255-256-257": ((255, 256, 257), 96), "100-300-513": ((100, 300, 513), 70)}
COLUMNS = {1, 63, 64, 65, 128, 129, 255, 256, 257, 513}


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


def make_pair(n, m, seed):
    """b starts as a mutated copy of a and goes on at random, so the distance depends on rows of every strip."""
    a = rand_seq(n, seed, 1)
    head = mutate(a, (0.02, 0.1, 0.3)[seed % 3], seed)[:m]
    b = head + rand_seq(m - len(head), seed, 2)
    assert len(a) == n and len(b) == m
    return a, b


def group_columns(lo, hi, count, rng):
    """`count` values of |a| in lo .. hi: hi itself, hi - 1, every chunk edge in the range and the column behind it, the rest at random."""
    must = [hi] + [c for c in (hi - 1, *range(64, hi, 64), *range(65, hi, 64)) if lo <= c < hi]
    must = list(dict.fromkeys(must))[:count]
    return must + [int(x) for x in rng.integers(lo, hi + 1, count - len(must))]


def make_batch(name, variant):
    """Group g of the batch has 1 + (g + variant) % 3 strips: over the three variants every group has one, two and three."""
    maxima, count = BATCHES[name]
    rng = np.random.default_rng(sum(maxima) * 3 + variant)
    spec, lo = [], 1
    for g, hi in enumerate(maxima):
        size = min(32, count - 32 * g)
        strips = 1 + (g + variant) % 3
        top = strips * STRIP if (g + variant) % 2 == 0 else max((strips - 1) * STRIP + 1, 777)  # the last row of a strip, or the first one (777: a strip not filled)
        rows = [top] + [1 + int(x) for x in rng.integers(0, top, size - 1)]
        spec += list(zip(group_columns(lo, hi, size, rng), rows, [strips] * size))
        lo = hi + 1
    pairs = [make_pair(n, m, 100 * variant + i) for i, (n, m, _) in enumerate(spec)]
    jobs = sum(1 + (g + variant) % 3 for g in range(len(maxima)))
    order = rng.permutation(len(pairs))  # the batch's own order is not the plan's
    return [pairs[i] for i in order], jobs


def run_twice(pa, monkeypatch, pairs, setting, grid):
    monkeypatch.setenv("PA_SLICE", str(setting))
    if grid is None:
        monkeypatch.delenv("PA_SLICE_GRID", raising=False)
    else:
        monkeypatch.setenv("PA_SLICE_GRID", str(grid))
    bt = pa.Batch(pairs)
    try:
        sh = dict(bt.shape())
        return sh, [np.asarray(bt.run()[0]).astype(np.int64) for _ in range(2)]
    finally:
        bt.close()


def test_the_batches_cover_the_columns():
    assert {hi for maxima, _ in BATCHES.values() for hi in maxima} >= COLUMNS
    assert all(64 <= count <= 96 for _, count in BATCHES.values()) and any(count % 32 for _, count in BATCHES.values())
    for name, (maxima, count) in BATCHES.items():
        for variant in range(3):
            pairs, _ = make_batch(name, variant)
            order = sorted(pairs, key=lambda p: len(p[0]))
            for g, hi in enumerate(maxima):
                grp = order[32 * g: 32 * g + 32]
                assert max(len(a) for a, _ in grp) == hi and -(-max(len(b) for _, b in grp) // STRIP) == 1 + (g + variant) % 3
                if hi - (maxima[g - 1] if g else 0) > 1:
                    assert len({len(a) for a, _ in grp}) > 1 and len({len(b) for _, b in grp}) > 1


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", list(BATCHES))
def test_ring_feed_against_oracle_and_strip_route(pa, oracle, monkeypatch, name, variant):
    pairs, jobs = make_batch(name, variant)
    want = np.array([oracle.nw_cost(a, b, True) for a, b in pairs], dtype=np.int64)
    sh0, other = run_twice(pa, monkeypatch, pairs, 0, None)
    assert not sh0["kernel"].startswith("pa::slice::"), sh0
    assert np.array_equal(other[0], want), "the strip route differs from the oracle"
    for grid in (None, 1):
        sh, passes = run_twice(pa, monkeypatch, pairs, R, grid)
        assert sh["kernel"] == f"pa::slice::slice_kernel<{R}>" and sh["sliced_rows_per_lane"] == R, sh
        assert sh["groups"] == 3 and sh["jobs"] == jobs, sh
        for k, got in enumerate(passes):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"grid {grid}, pass {k}: " + ", ".join(
                f"#{i} |a|={len(pairs[i][0])} |b|={len(pairs[i][1])}: {int(got[i])} != {int(want[i])}" for i in bad[:8])
            assert np.array_equal(got, other[0]), f"grid {grid}, pass {k} differs from the PA_SLICE=0 route"
