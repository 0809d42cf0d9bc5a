"""The bit-sliced kernel under every ticket order of its (group, strip) jobs (csrc/slice_job_order.hpp: bands of PA_SLICE_CHAIN strips of
every group) and with fewer wavefronts than jobs (PA_SLICE_GRID), so that the order decides which strips run beside their producer and
which long after it: with a grid of 1 the jobs run strictly in ticket order, with 2 a consumer runs beside or after its producer.

PA_SLICE = 28 (strips of 1792 rows).  96 pairs = 3 groups, |a| ragged in 65 .. 200, |b| ragged in 1 .. 8193: the groups have 5, 3 and 1
strips, one pair's |b| is 7169 (the first row of strip 5).  Every distance against oracle.levenshtein and against the PA_SLICE=0 route;
each batch runs twice on its resident plan: the second pass depends on the strips having handed their boundary rows back reset, whatever
the order.  A second batch has 66 groups of one strip and one group of five."""
import numpy as np
import pytest

from tests.util_seq import mutate, rand_seq

pytestmark = pytest.mark.gpu

R = 28
STRIP = 64 * R


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


def three_groups():
    """The groups are cut by |a| (ascending), so |a| decides a pair's group: 65 .. 109 -> |b| up to 1792 (1 strip), 110 .. 154 -> up to
    4 * 1792 - 1000 (3 .. 4 strips: 3 here), 155 .. 200 -> up to 8193 (5 strips)."""
    pairs = []
    for i in range(96):
        g = i // 32
        n = (65, 110, 155)[g] + (i * 7) % 45 + (1 if g == 2 and i == 95 else 0)
        top = (STRIP, 3 * STRIP, 8193)[g]
        m = 1 + (i * 2654435761) % top
        pairs.append([n, m])
    pairs[0][1] = 1
    pairs[31][1] = STRIP          # the last row of strip 1: the group keeps one strip
    pairs[40][1] = 2 * STRIP + 1  # the first row of strip 3
    pairs[63][1] = 3 * STRIP
    pairs[70][1] = 4 * STRIP + 1  # 7169: the first row of strip 5
    pairs[95][1] = 8193
    pairs[80][1] = 4 * STRIP      # the last row of strip 4
    out = [make_pair(n, m, 5000 + i) for i, (n, m) in enumerate(pairs)]
    order = np.random.default_rng(12).permutation(len(out))  # the batch's own order is not the plan's
    return [out[i] for i in order]


def many_groups():
    """66 groups of one strip (|a| 65 .. 130, |b| 1 .. 300) and one group of five (|a| 150 .. 181, |b| up to 8193, one of them 7169)."""
    spec = [(65 + i % 66, 1 + (i * 2654435761) % 300) for i in range(66 * 32)]
    spec += [(150 + i, (7169, 8193, 1, STRIP + 1)[i] if i < 4 else 1 + (i * 2654435761) % 8193) for i in range(32)]
    return [make_pair(n, m, 9000 + i) for i, (n, m) in enumerate(spec)]


_cache = {}


def reference(name, pa, oracle, monkeypatch):
    """-> (pairs, oracle distances, distances of the PA_SLICE=0 route), made once per batch."""
    if name not in _cache:
        pairs = {"three": three_groups, "many": many_groups}[name]()
        want = np.array([oracle.levenshtein(a, b) for a, b in pairs], dtype=np.int64)
        with monkeypatch.context() as mp:
            mp.setenv("PA_SLICE", "0")
            bt = pa.Batch(pairs)
            try:
                assert not bt.shape()["kernel"].startswith("pa::slice::"), bt.shape()
                other = np.asarray(bt.run()[0]).astype(np.int64)
            finally:
                bt.close()
        _cache[name] = (pairs, want, other)
    return _cache[name]


def run_sliced(pa, monkeypatch, pairs, chain, grid, groups, jobs, want, other):
    monkeypatch.setenv("PA_SLICE", str(R))
    for var, val in (("PA_SLICE_CHAIN", chain), ("PA_SLICE_GRID", grid)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    bt = pa.Batch(pairs)
    try:
        sh = bt.shape()
        assert sh["kernel"] == f"pa::slice::slice_kernel<{R}>" and sh["sliced_rows_per_lane"] == R, sh
        assert sh["groups"] == groups and sh["jobs"] == jobs, sh
        passes = [np.asarray(bt.run()[0]).astype(np.int64) for _ in range(2)]
    finally:
        bt.close()
    for k, got in enumerate(passes):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"pass {k}: " + ", ".join(f"#{i} |a|={len(pairs[i][0])} |b|={len(pairs[i][1])}: {int(got[i])} != {int(want[i])}" for i in bad[:8])
        assert np.array_equal(got, other), f"pass {k} differs from the PA_SLICE=0 route"


@pytest.mark.parametrize("grid", [None, 1, 2])
@pytest.mark.parametrize("chain", [None, 0, 1, 2, 3])
def test_three_groups_every_order(pa, oracle, monkeypatch, chain, grid):
    pairs, want, other = reference("three", pa, oracle, monkeypatch)
    strips = sorted({-(-len(b) // STRIP) for _, b in pairs})
    assert strips == [1, 2, 3, 4, 5] and any(len(b) == 7169 for _, b in pairs)
    assert all(65 <= len(a) <= 200 and 1 <= len(b) <= 8193 for a, b in pairs)
    run_sliced(pa, monkeypatch, pairs, chain, grid, 3, 5 + 3 + 1, want, other)


def test_one_long_group_among_many_short_ones(pa, oracle, monkeypatch):
    pairs, want, other = reference("many", pa, oracle, monkeypatch)
    run_sliced(pa, monkeypatch, pairs, 1, 3, 67, 66 + 5, want, other)
