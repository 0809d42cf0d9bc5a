"""The batched gap-affine kernel (pa_affine_batch_*, csrc/affine_kernel.hpp) against the plain DP of tests/affine_plain.py: cost and
exact CIGAR string of every pair, plus an independent pricing of the CIGAR, at the kernel's shape edges (segment widths, strip counts),
over every reference constructor and any byte."""
import os

import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost
from tests import affine_plain as ap

pytestmark = pytest.mark.gpu

R = pa.capi.AFFINE_ROWS_PER_LANE
MODELS = {
    "lcs": AffineCost.lcs(),
    "unit": AffineCost.unit(),
    "linear": AffineCost.linear(3, 2),
    "linear_asymmetric": AffineCost.linear_asymmetric(2, 1, 3),
    "affine": AffineCost.affine(4, 6, 2),
    "linear_affine": AffineCost.linear_affine(3, 2, 4, 1),
    "affine_asymmetric": AffineCost.affine_asymmetric(5, 3, 1, 7, 2),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


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


def check(pairs, cm, results):
    assert len(results) == len(pairs)
    for p, ((x, y), (c, g)) in enumerate(zip(pairs, results)):
        wc, wg = ap.affine_nw(x, y, cm)
        assert (c, g) == (wc, wg), (p, len(x), len(y))
        assert ap.affine_verify(g, x, y, cm) == c
        assert ap.no_adjacent_same_op(g)


def traced(pairs, cm):
    b = AffineBatch(pairs, cm, trace=True)
    try:
        res = b.align()
        costs = b.run()
    finally:
        b.close()
    assert costs.tolist() == [c for c, _ in res]
    return res


EDGE_M = [0, 1, 2, R - 1, R, R + 1, 2 * R, 2 * R + 1, 4 * R + 3, 8 * R, 8 * R + 1, 16 * R + 5, 32 * R, 32 * R + 1, 64 * R - 1, 64 * R,
          64 * R + 1, 128 * R, 128 * R + 1, 128 * R + 77]


def edge_pairs(seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for k, m in enumerate(EDGE_M):
        y = rand_seq(rng, m)
        n = (0, 1, max(m // 2, 1), m + 3, 40)[k % 5]
        x = mutate(rng, y, 0.1)[:n] if k % 2 else rand_seq(rng, n)
        pairs.append((x, y))
        pairs.append((y[: min(m, 30)], rand_seq(rng, (3 * k) % 37)))
    return pairs


@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_constructor_at_the_shape_edges(name):
    pairs = edge_pairs(len(name))
    check(pairs, MODELS[name], traced(pairs, MODELS[name]))


def test_lopsided_homopolymers_and_divergence():
    rng = np.random.default_rng(5)
    pairs = [(b"A" * 5, rand_seq(rng, 900)), (rand_seq(rng, 900), b"C" * 3), (b"A" * 300, b"A" * 290 + b"C" * 4), (b"AC" * 200, b"A" * 400),
             (b"G" * 1500, b"G" * 1500), (b"T" * 700, b"T" * 1300)]
    for k, d in enumerate((0.01, 0.05, 0.1, 0.2, 0.3)):
        y = rand_seq(rng, 300 + 250 * k)
        pairs.append((mutate(rng, y, d), y))
    for cm in (AffineCost.affine(4, 6, 2), AffineCost.linear_affine(3, 2, 4, 1), AffineCost.affine_asymmetric(5, 3, 1, 7, 2)):
        check(pairs, cm, traced(pairs, cm))


def test_any_byte():
    rng = np.random.default_rng(6)
    protein = b"ACDEFGHIKLMNPQRSTVWY"
    pairs = []
    for k in range(6):
        y = rand_seq(rng, 40 + 90 * k, protein)
        pairs.append((mutate(rng, y, 0.15, protein), y))
    y = bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    pairs.append((mutate(rng, y, 0.1, bytes(range(256))), y))
    pairs.append((b"\x00\xff" * 40, b"\xff\x00" * 41))
    pairs.append((b"acgtnNACGT" * 20, b"ACGTNnacgt" * 19))
    for cm in (AffineCost.affine(4, 6, 2), AffineCost.unit(), AffineCost.lcs()):
        check(pairs, cm, traced(pairs, cm))


def mixed(seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(160):
        m = int(rng.choice([0, 5, 30, 100, 200, 600, 1024, 1500, 2500]))
        y = rand_seq(rng, m)
        pairs.append((mutate(rng, y, 0.08), y))
    return pairs


def test_mixed_batch_shuffled_reversed_twice():
    cm = AffineCost.affine(4, 6, 2)
    pairs = mixed(7)
    base = traced(pairs, cm)
    check(pairs, cm, base)
    perm = np.random.default_rng(8).permutation(len(pairs))
    sh = traced([pairs[i] for i in perm], cm)
    assert sh == [base[i] for i in perm]
    assert traced(pairs[::-1], cm) == base[::-1]
    b = AffineBatch(pairs, cm)
    assert b.run().tolist() == b.run().tolist() == [c for c, _ in base]
    b.close()


def test_unit_costs_equal_the_bitpacked_batch():
    rng = np.random.default_rng(9)
    pairs = [pa.generate.generate_pair(int(n), e, seed=50 + k) for k, (n, e) in enumerate(zip(rng.integers(1, 3000, 40), np.tile([0.01, 0.1, 0.3], 14)))]
    b = AffineBatch(pairs, AffineCost.unit())
    got = b.run()
    b.close()
    want, _ = pa.Batch(pairs).run()
    assert got.tolist() == want.tolist()


def test_budget_chunks_give_the_same_result(monkeypatch):
    cm = AffineCost.linear_affine(3, 2, 4, 1)
    pairs = mixed(10)[:60]
    b = AffineBatch(pairs, cm, trace=True)
    one = b.align()
    assert b.info()["trace_chunks"] == 1
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "12")  # the largest pair needs 7.3 MB, all 68 MB
    several = b.align()
    chunks = b.info()["trace_chunks"]
    b.close()
    assert chunks >= 6 and several == one


def plan_model(pairs):
    """waves, packed pairs, strip pairs, lane use of the planner: 64 / g packed pairs of one width g per wave, a wave per longer pair."""
    per_g, strip, lanes, slots = {}, 0, 0, 0
    for _, y in pairs:
        m = len(y)
        lanes += -(-max(m, 1) // R)
        if m <= 64 * R:
            g = 1
            while g * R < m:
                g *= 2
            per_g[g] = per_g.get(g, 0) + 1
        else:
            strip += 1
            slots += 64 * -(-m // (64 * R))
    waves = strip
    for g, c in per_g.items():
        w = -(-c // (64 // g))
        waves += w
        slots += 64 * w
    return waves, sum(per_g.values()), strip, lanes / slots


def test_info_matches_the_plan_model():
    pairs = mixed(11) + edge_pairs(12)
    b = AffineBatch(pairs, AffineCost.unit())
    info = b.info()
    b.close()
    waves, packed, strip, use = plan_model(pairs)
    assert (info["waves"], info["packed_pairs"], info["strip_pairs"]) == (waves, packed, strip)
    assert info["lane_use"] == pytest.approx(use)
    assert info["trace_chunks"] == 0


def test_rejected_arguments(monkeypatch):
    for cm in (AffineCost(0, 1, 1), AffineCost.linear(1, 1001), AffineCost(1, None, 1), AffineCost.double_affine(4, 6, 2, 20, 1)):
        with pytest.raises(ValueError):
            AffineBatch([(b"ACGT", b"ACGT")], cm)
    with pytest.raises(ValueError):
        AffineBatch([(b"A", b"A"), (b"A" * 600000, b"C" * 600000)], AffineCost.linear(1000, 1000))
    b = AffineBatch([(b"ACGT", b"ACGT")], AffineCost.unit())
    with pytest.raises(ValueError):  # created without trace
        b.align()
    b.close()
    b = AffineBatch([(b"ACGT" * 10, b"ACGT" * 10), (b"A" * 3000, b"A" * 3000)], AffineCost.unit(), trace=True)
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
    with pytest.raises(ValueError, match="pair 1"):
        b.align()
    b.close()


def test_long_pairs():
    rng = np.random.default_rng(13)
    cm = AffineCost.affine(4, 6, 2)
    pairs = []
    for k, d in enumerate((0.02, 0.1)):
        y = rand_seq(rng, 10000 + 37 * k)
        pairs.append((mutate(rng, y, d), y))
    check(pairs, cm, traced(pairs, cm))
    y = rand_seq(rng, 25000)
    x = mutate(rng, y, 0.05)
    b = AffineBatch([(x, y), (y[:4000], x[:3000])], AffineCost.linear_affine(3, 2, 4, 1))
    got = b.run().tolist()
    b.close()
    assert got == [ap.affine_nw(x, y, AffineCost.linear_affine(3, 2, 4, 1), trace=False)[0],
                   ap.affine_nw(y[:4000], x[:3000], AffineCost.linear_affine(3, 2, 4, 1), trace=False)[0]]


def test_align_affine_convenience():
    pairs = [(b"ACGTTGCA", b"ACGTGCA"), (b"", b"AC"), (b"AC", b"")]
    cm = AffineCost.affine(4, 6, 2)
    check(pairs, cm, pa.align_affine(pairs, cm))


ROUTE_MODELS = {
    "affine": AffineCost.affine(4, 6, 2),
    "unit": AffineCost.unit(),
    # deletions go through the delete layer only (no linear deletion edge), insertions have both edges
    "delete_layer_only": AffineCost(3, 2, None, [("ins", 4, 1), ("del", 5, 2)]),
}
# (|a|, |b|): empty b, empty a; segment width 1 and 2; 1024 rows are the widest packed pair, 1025 the first with two strips (and the first
# that is chained); |a| = 63, 64, 65 around the chained kernel's 64-column chunk and the first column checkpoint of 64-column tiles;
# |a| = 129 has two column checkpoints (packed, chained, and in a narrow segment)
ROUTE_SHAPES = [(5, 0), (0, 7), (20, 16), (20, 17), (129, 1024), (129, 1025), (63, 2049), (64, 2049), (65, 2049), (129, 300)]


@pytest.fixture(scope="module")
def route_pairs():
    rng = np.random.default_rng(14)
    pairs = []
    for n, m in ROUTE_SHAPES:
        y = rand_seq(rng, m)
        off = int(rng.integers(0, max(m - n, 0) + 1))
        x = (mutate(rng, y[off:off + n], 0.1) + rand_seq(rng, n))[:n]
        pairs.append((x, y))
    assert [(len(x), len(y)) for x, y in pairs] == ROUTE_SHAPES
    return pairs


@pytest.mark.parametrize("name", sorted(ROUTE_MODELS))
def test_all_four_routes_agree(name, route_pairs):
    """One batch through run(), align(), align_tiled(64) and align_tiled(64) with chained strips: the costs and CIGARs of the plain DP
    from each of them."""
    cm = ROUTE_MODELS[name]
    want = [ap.affine_nw(x, y, cm) for x, y in route_pairs]
    b = AffineBatch(route_pairs, cm, trace=True)
    try:
        assert b.run().tolist() == [c for c, _ in want]
        assert b.align() == want
        assert b.align_tiled(64) == want
        b.set_chain(True)
        assert b.align_tiled(64) == want
        assert b.chain_info()["chain_pairs"] == sum(m > 64 * R for _, m in ROUTE_SHAPES) == 4
        assert b.run().tolist() == [c for c, _ in want]
    finally:
        b.close()
