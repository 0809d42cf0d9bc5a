"""A bit-sliced batch builds its bit planes straight from the uploaded sequences (csrc/slice_kernel.hpp: slice_pack_a_kernel reads 16 bases
per lane, slice_pack_b_kernel two pieces of 16); the strip kernels still go through the encode kernels (codes and profile), so the same
pairs under PA_SLICE=0 are the reference here.

Lengths: |a| mod 16 in {0, 1, 15} and |b| mod 64 in {0, 1, 15, 16, 17, 31, 32, 33, 63} (a piece that is full, holds one base, lacks one,
and a second piece / second half that is absent, starts, is full), all 27 combinations twice and then some: 70 pairs, so the last
group has 6 pairs; the batch's last pair ends both concatenated buffers, its b in the last 16 bytes.

Then one byte outside ACGT, and separately one lowercase base, at the piece edges of a (0, 15, 16, len - 1) and of b (0, 15, 16, 31, 32,
len - 1) of the first, the 32nd and the last pair: both routes must give the same status -- invalid base, or success with equal costs."""
import random

import numpy as np
import pytest

from tests.util_seq import mutate, rand_seq

pytestmark = pytest.mark.gpu

A_MOD = (0, 1, 15)
B_MOD = (0, 1, 15, 16, 17, 31, 32, 33, 63)
PAIRS = 70


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


@pytest.fixture(scope="module")
def pairs():
    rng = random.Random(49)
    combos = [(ra, rb) for ra in A_MOD for rb in B_MOD]
    out = []
    for i in range(PAIRS):
        ra, rb = combos[i % len(combos)]
        n, m = 16 * rng.randint(3, 12) + ra, 64 * rng.randint(1, 4) + rb
        if i == PAIRS - 1:
            n, m = 16 * 5, 64 * 2 + 16  # the last pair fills its last pieces: a and b end with the buffers
        a = rand_seq(n, 7000 + i, 1)
        head = mutate(a, (0.02, 0.1, 0.3)[i % 3], 7000 + i)[:m]
        out.append((a, head + rand_seq(m - len(head), 7000 + i, 2)))
        assert len(out[-1][0]) == n and len(out[-1][1]) == m and n > 33 and m > 33
    assert {len(a) % 16 for a, _ in out} == set(A_MOD) and {len(b) % 64 for _, b in out} == set(B_MOD)
    return out


def status(pa, monkeypatch, setting, ps):
    """("ok", costs) or ("invalid base",) of the batch under PA_SLICE=<setting>, and whether it ran bit-sliced."""
    monkeypatch.setenv("PA_SLICE", str(setting))
    bt = pa.Batch(ps)
    try:
        sh = bt.shape()
        sliced = sh["kernel"].startswith("pa::slice::slice_kernel<")
        assert sliced == (setting != 0), sh
        if sliced:
            assert sh["sliced_rows_per_lane"] == setting and sh["groups"] == -(-len(ps) // 32), sh
        try:
            costs, _ = bt.run()
        except ValueError as e:
            assert "outside ACGT" in str(e)
            return ("invalid base",)
        return ("ok", costs.tolist())
    finally:
        bt.close()


def test_costs_equal_the_strip_route(pa, oracle, monkeypatch, pairs):
    ref = status(pa, monkeypatch, 0, pairs)
    got = status(pa, monkeypatch, 49, pairs)
    assert ref[0] == "ok" and got == ref
    assert ref[1] == [oracle.levenshtein(a, b) for a, b in pairs]  # (and the reference route is right itself)


@pytest.mark.parametrize("byte", [b"N", b"a"], ids=["outside_ACGT", "lowercase"])
def test_one_bad_byte_at_the_piece_edges(pa, monkeypatch, pairs, byte):
    seen = set()
    for which in (0, 31, PAIRS - 1):
        a, b = pairs[which]
        spots = [("a", k) for k in (0, 15, 16, len(a) - 1)] + [("b", k) for k in (0, 15, 16, 31, 32, len(b) - 1)]
        for side, k in spots:
            s = a if side == "a" else b
            bad = s[:k] + byte + s[k + 1:]
            assert len(bad) == len(s) and bad != s
            ps = list(pairs)
            ps[which] = (bad, b) if side == "a" else (a, bad)
            ref = status(pa, monkeypatch, 0, ps)
            got = status(pa, monkeypatch, 49, ps)
            assert got == ref, (which, side, k, got[0], ref[0])
            seen.add(ref[0])
    if byte == b"N":
        assert seen == {"invalid base"}, seen  # (the encode kernels flag it wherever it stands)
