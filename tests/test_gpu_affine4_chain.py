"""The chained double-affine route (Affine4Batch.set_chain: a wavefront per strip of 1024 rows, the strips of a pair chained through
their boundary rows, every 16-byte value handed over as two 8-byte halves) against the plain DP of tests/affine4_plain.py and against
the unchained routes of the same batch: the strip edges and the ends of the 64-column load chunk, every model, runs of both insert
layers and of the delete layers carried through the hand-off, a mixed batch run again and again, more jobs than the chip holds
wavefronts, the memory budget, and costs at 1000 with totals next to 2^30."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineCost
from tests import affine4_plain as a4
from tests import affine_heavy_cases as heavy
from tests.affine_heavy_cases import runs_of
from tests.test_gpu_affine4 import MODELS, mixed, mutate, rand_seq

pytestmark = pytest.mark.gpu

DOUBLE = MODELS["double_affine"]
EDGE_M = (1025, 2048, 2049, 3072, 3073, 5000)
EDGE_N = (0, 1, 63, 64, 65, 127, 128, 129, 300)  # the ends of the 64-column load chunk, and the single-value row
VALUE = 16  # bytes of one boundary value {M, I1, I2, 0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def edge_pairs():
    """EDGE_M[q] meets EDGE_N[(3 q + k) % 9] for k = 0, 1, 2 (tests/test_gpu_affine_chain.edge_pairs): 18 pairs, every |a| twice; odd
    ones mutated copies, even ones random."""
    rng = np.random.default_rng(31)
    pairs = []
    for q, m in enumerate(EDGE_M):
        for k in range(3):
            n = EDGE_N[(3 * q + k) % 9]
            y = rand_seq(rng, m)
            if len(pairs) % 2:
                off = int(rng.integers(0, m - n + 1))
                x = (mutate(rng, y[off:off + n], 0.1) + rand_seq(rng, n))[:n]
            else:
                x = rand_seq(rng, n)
            assert len(x) == n
            pairs.append((x, y))
    return pairs


@pytest.fixture(scope="module")
def edges():
    pairs = edge_pairs()
    return pairs, [a4.affine4_nw(x, y, DOUBLE) for x, y in pairs]


def strips(pairs):
    return sum(-(-len(y) // 1024) for _, y in pairs if len(y) > 1024)


def row_bytes(pairs):
    return sum((-(-len(y) // 1024) - 1) * (len(x) + 1) * VALUE for x, y in pairs if len(y) > 1024)


def test_strip_and_chunk_edges(edges):
    pairs, want = edges
    assert sorted({len(x) for x, _ in pairs}) == sorted(EDGE_N) and len(pairs) == 18
    b = Affine4Batch(pairs, DOUBLE, trace=True)
    try:
        plain, jobs = {}, {}
        for C in (64, 1024):
            plain[C] = b.align_tiled(C)
            jobs[C] = b.tiled_info()["tile_jobs"]
        b.set_chain(True)
        assert b.chain_info()["on"]
        assert b.run().tolist() == [c for c, _ in want]
        assert b.chain_info() == {"on": True, "chain_pairs": 18, "chain_jobs": strips(pairs), "chunks": 1, "bnd_bytes_max": row_bytes(pairs)}
        for C in (64, 1024):
            got = b.align_tiled(C)
            for p, (w, r) in enumerate(zip(want, got)):
                assert r == w, (C, p, len(pairs[p][0]), len(pairs[p][1]))
            assert got == plain[C]
            assert b.tiled_info()["tile_jobs"] == jobs[C]
            assert b.chain_info()["chain_jobs"] == strips(pairs)
    finally:
        b.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_model(name, edges):
    pairs = [edges[0][k] for k in (0, 4, 5, 7, 10, 14)]  # |b| = 1025, 2048 (twice), 2049, 3072, 3073
    assert [len(y) for _, y in pairs] == [1025, 2048, 2048, 2049, 3072, 3073]
    cm = MODELS[name]
    want = [a4.affine4_nw(x, y, cm) for x, y in pairs]
    b = Affine4Batch(pairs, cm, trace=True, chain=True)
    try:
        assert b.run().tolist() == [c for c, _ in want]
        assert b.align_tiled(64) == want
    finally:
        b.close()


HAND_OFF = {"double_affine": (30, 84, 84), "linear_edges": (24, 72, 72)}  # 6 + 12 * 2, 24 + 60; 12 + 12, 12 + 60


@pytest.mark.parametrize("name", sorted(HAND_OFF))
def test_both_pieces_through_the_hand_off(name):
    """Insertion runs that are open across rows 1024 and 2048, in the first piece (12 bytes under double_affine) and in the second, and
    a deletion run open across column 64, the end of the first load chunk."""
    cm = MODELS[name]
    rng = np.random.default_rng(21)
    x = rand_seq(rng, 2100)
    gap = lambda L: rand_seq(rng, L, b"NRYK")  # noqa: E731  bytes x does not have: the gap has one best place
    cuts = ((1018, 12, 1024), (1000, 60, 1024), (2030, 60, 2048))
    pairs = [(x, x[:at] + gap(L) + x[at:]) for at, L, _ in cuts]
    pairs.append((x[:34] + gap(60) + x[34:], x))  # columns 35 .. 94 of a deleted
    want = [a4.affine4_nw(a, b, cm) for a, b in pairs]
    for (at, L, row), (cost, cigar), c in zip(cuts, want, HAND_OFF[name]):
        runs = [(p0[1], p1[1]) for p0, p1 in runs_of(cigar, "I")]
        assert runs == [(at, at + L)] and at < row < at + L, cigar  # one run, open at the strip's last row
        assert cost == c
    assert [(p0[0], p1[0]) for p0, p1 in runs_of(want[3][1], "D")] == [(34, 94)]  # ... and one open at column 64
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        plain = b.align_tiled()
        b.set_chain(True)
        assert b.run().tolist() == [c for c, _ in want]
        assert b.align_tiled() == want == plain
        assert b.align_tiled(64) == want
    finally:
        b.close()
    b = Affine4Batch(pairs, cm, trace=True, chain=True)  # from the constructor
    try:
        assert b.chain_info()["on"]
        assert b.align_tiled() == want
        assert b.chain_info()["chain_pairs"] == 4
    finally:
        b.close()


def test_mixed_batch_on_off_and_again():
    pairs = mixed(17) + [(b"", b""), (b"", rand_seq(np.random.default_rng(1), 1500)), (b"ACGT", b"")]
    long_ = [(x, y) for x, y in pairs if len(y) > 1024]
    assert long_ and len(long_) < len(pairs)
    off = {"on": False, "chain_pairs": 0, "chain_jobs": 0, "chunks": 0, "bnd_bytes_max": 0}
    b = Affine4Batch(pairs, DOUBLE, trace=True)
    try:
        info = b.info()
        costs = b.run().tolist()
        traced = b.align_tiled(256)
        assert b.chain_info() == off
        b.set_chain(True)
        assert b.info() == info
        assert b.run().tolist() == costs
        ci = b.chain_info()
        assert (ci["on"], ci["chain_pairs"], ci["chain_jobs"], ci["chunks"]) == (True, len(long_), strips(pairs), 1)
        assert ci["bnd_bytes_max"] == row_bytes(pairs)
        assert b.run().tolist() == costs  # the rows are reset before every pass
        assert b.align_tiled(256) == traced
        assert b.run().tolist() == costs  # ... and after a traced pass, which keeps rows of its own
        b.set_chain(False)
        assert b.run().tolist() == costs and b.info() == info
        b.set_chain(True)
        assert b.run().tolist() == costs
        assert b.chain_info()["chain_jobs"] == strips(pairs)
        assert b.align() == traced  # the untiled route ignores the setting
    finally:
        b.close()
    assert traced[0] == a4.affine4_nw(*pairs[0], DOUBLE)
    b = Affine4Batch(pairs, DOUBLE)  # the counters stay zero while the setting is off
    try:
        assert b.run().tolist() == costs and b.chain_info() == off
    finally:
        b.close()


def compute_units():
    """multiProcessorCount of device 0, asked of the HIP runtime the library has loaded."""
    import ctypes

    pa.capi.load()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    v = ctypes.c_int(0)
    assert ctypes.CDLL(path).hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    assert 8 <= v.value <= 1024 and v.value % 8 == 0, v.value  # (MI355X: 256, 32 on each of 8 XCDs)
    return v.value


def test_more_jobs_than_resident_wavefronts():
    resident = 32 * compute_units()  # 4 SIMDs with 8 wavefronts each at the most
    m, per_pair = 12300, 13
    npairs = -(-2 * resident // per_pair) + 1
    rng = np.random.default_rng(41)
    letters = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for k in range(npairs):
        n = 40 + k % 161
        y = letters[rng.integers(0, 4, m)]
        off = int(rng.integers(0, m - n))
        x = y[off:off + n].copy()
        flip = rng.random(n) < 0.1
        x[flip] = letters[rng.integers(0, 4, int(flip.sum()))]
        pairs.append((x.tobytes(), y.tobytes()))
    b = Affine4Batch(pairs, DOUBLE)
    try:
        plain = b.run().tolist()
        b.set_chain(True)
        got = b.run().tolist()
        ci = b.chain_info()
    finally:
        b.close()
    assert ci["chain_pairs"] == npairs and ci["chain_jobs"] == per_pair * npairs >= 2 * resident and ci["chunks"] == 1
    assert got == plain
    assert got[:8] == [a4.affine4_nw(x, y, DOUBLE)[0] for x, y in pairs[:8]]


def test_budget(monkeypatch):
    rng = np.random.default_rng(51)
    letters = np.frombuffer(b"ACGT", np.uint8)

    def pair(n, m):
        y = letters[rng.integers(0, 4, m)]
        x = letters[rng.integers(0, 4, n)]
        x[:m] = np.where(rng.random(m) < 0.1, x[:m], y)  # a noisy copy of y, then a random tail
        return x.tobytes(), y.tobytes()

    pairs = [pair(20000, 4097) for _ in range(8)]  # 5 strips: 4 rows of 20 001 values, 1.28 MB
    b = Affine4Batch(pairs, DOUBLE)
    try:
        plain = b.run().tolist()
        b.set_chain(True)
        one = b.run().tolist()
        assert b.chain_info()["chunks"] == 1 and b.chain_info()["bnd_bytes_max"] == 8 * 4 * 20001 * VALUE
        monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "2")
        several = b.run().tolist()
        ci = b.chain_info()
    finally:
        b.close()
    assert ci["chunks"] >= 4 and ci["bnd_bytes_max"] <= 2 << 20 and ci["chain_jobs"] == 40
    assert several == one == plain
    big = [pairs[0], pair(40000, 4097)]  # 2.56 MB of rows
    b = Affine4Batch(big, DOUBLE, chain=True)
    try:
        with pytest.raises(ValueError, match="pa_affine4_batch_run: pair 1"):
            b.run()
        assert "chained route" in pa.capi.last_error()
        b.set_chain(False)
        got = b.run().tolist()
        monkeypatch.delenv("PA_AFFINE_TRACE_BUDGET_MB")
        b.set_chain(True)
        assert b.run().tolist() == got and got[0] == plain[0]
    finally:
        b.close()


@pytest.mark.parametrize("name", sorted(heavy.THIN_MODELS4))
def test_heavy_costs_and_totals_next_to_the_limit(name):
    """Costs at 1000, the largest a batch takes, and the two thin pairs of a million rows whose totals lie within 0.2 % of 2^30: their
    thousand boundary rows hold M next to kInf and layer values above it, the top of what a half can carry."""
    cm = heavy.THIN_MODELS4[name]
    assert heavy.create_max_edge(cm) == 1000
    thin, exp = heavy.thin_limit(cm), heavy.thin_expected(cm)
    rng = np.random.default_rng(61)
    y = rand_seq(rng, 2500)
    pairs = heavy.ordinary() + [thin[1], thin[3], (mutate(rng, y, 0.08), y)]
    assert all(len(b) > 1024 for _, b in pairs[3:]) and all(heavy.LIMIT - heavy.LIMIT // 500 <= c < heavy.LIMIT for c, _ in (exp[1], exp[3]))
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        costs = b.run().tolist()
        plain = b.align_tiled(64)
        b.set_chain(True)
        assert b.run().tolist() == costs
        assert b.chain_info()["chain_pairs"] == 3
        assert b.align_tiled(64) == plain
    finally:
        b.close()
    assert plain[3] == exp[1] and plain[4] == exp[3] and costs == [c for c, _ in plain]
    assert plain[0] == a4.affine4_nw(*pairs[0], cm)
