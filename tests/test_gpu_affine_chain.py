"""The chained gap-affine route (AffineBatch.set_chain: a wavefront per strip of 1024 rows, the strips of a pair chained through their
boundary rows) against the plain DP of tests/affine_plain.py and against the unchained routes: the strip edges and the ends of the
64-column load chunk, every cost-model constructor, an insertion run carried through the hand-off, a mixed batch run again and again,
more jobs than the chip holds wavefronts, and the memory budget."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost
from tests import affine_plain as ap
from tests.test_gpu_affine import MODELS, mixed, mutate, rand_seq
from tests.test_gpu_affine_tiled import runs_of

pytestmark = pytest.mark.gpu

EDGE_M = (1025, 2048, 2049, 3072, 3073, 5000)
EDGE_N = (0, 1, 63, 64, 65, 127, 128, 129, 300)  # the ends of the 64-column load chunk, and the single-value row


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def edge_pairs():
    """EDGE_M[q] meets EDGE_N[(3 q + k) % 9] for k = 0, 1, 2: 18 pairs, every |a| twice; odd ones mutated copies, even ones random."""
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
    cm = AffineCost.affine(4, 6, 2)
    return pairs, cm, [ap.affine_nw(x, y, cm) for x, y in pairs]


def strips(pairs):
    return sum(-(-len(y) // 1024) for _, y in pairs if len(y) > 1024)


def test_strip_and_chunk_edges(edges):
    pairs, cm, want = edges
    assert sorted({len(x) for x, _ in pairs}) == sorted(EDGE_N) and len(pairs) == 18
    b = AffineBatch(pairs, cm, trace=True)
    try:
        plain = {C: b.align_tiled(C) for C in (64, 1024)}
        jobs = {}
        for C in (64, 1024):
            b.align_tiled(C)
            jobs[C] = b.tiled_info()["tile_jobs"]
        b.set_chain(True)
        assert b.chain_info()["on"]
        assert b.run().tolist() == [c for c, _ in want]
        assert b.chain_info() == {"on": True, "chain_pairs": 18, "chain_jobs": strips(pairs), "chunks": 1,
                                  "bnd_bytes_max": sum((-(-len(y) // 1024) - 1) * (len(x) + 1) * 8 for x, y in pairs)}
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
def test_every_constructor(name, edges):
    pairs = [edges[0][k] for k in (0, 4, 5, 7, 10, 14)]  # |b| = 1025, 2048 (twice), 2049, 3072, 3073
    cm = MODELS[name]
    want = [ap.affine_nw(x, y, cm) for x, y in pairs]
    b = AffineBatch(pairs, cm, trace=True, chain=True)
    try:
        assert b.run().tolist() == [c for c, _ in want]
        assert b.align_tiled(64) == want
    finally:
        b.close()


@pytest.mark.parametrize("cm", (AffineCost.affine(4, 6, 2), AffineCost.linear_affine(3, 2, 4, 1)), ids=("affine", "linear_affine"))
def test_insertion_run_through_the_hand_off(cm):
    rng = np.random.default_rng(21)
    x = rand_seq(rng, 2100)
    pairs = [(x, x[:1000] + rand_seq(rng, 60) + x[1000:])]
    want = [ap.affine_nw(*pairs[0], cm)]
    runs = [(j0, j1) for (_, j0), (_, j1) in runs_of(want[0][1], "I") if j0 < 1024 < j1]
    assert len(runs) == 1, want[0][1]  # one run that starts above row 1024 and ends below it: I is open at the strip's last row
    b = AffineBatch(pairs, cm, trace=True, chain=True)
    try:
        assert b.run().tolist() == [want[0][0]]
        assert b.align_tiled() == want
        assert pa.align_affine(pairs, cm, tiled=True, chain=True) == want
    finally:
        b.close()


def test_mixed_batch_on_off_and_again():
    cm = AffineCost.affine(4, 6, 2)
    pairs = mixed(17) + [(b"", b""), (b"", rand_seq(np.random.default_rng(1), 1500)), (b"ACGT", b"")]
    long_ = [(x, y) for x, y in pairs if len(y) > 1024]
    assert long_ and len(long_) < len(pairs)
    b = AffineBatch(pairs, cm, trace=True)
    try:
        info = b.info()
        costs = b.run().tolist()
        traced = b.align_tiled(256)
        assert b.chain_info() == {"on": False, "chain_pairs": 0, "chain_jobs": 0, "chunks": 0, "bnd_bytes_max": 0}
        b.set_chain(True)
        assert b.info() == info
        assert b.run().tolist() == costs
        ci = b.chain_info()
        assert (ci["on"], ci["chain_pairs"], ci["chain_jobs"], ci["chunks"]) == (True, len(long_), strips(pairs), 1)
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
    cm = AffineCost.unit()
    b = AffineBatch(pairs, cm)
    try:
        plain = b.run().tolist()
        b.set_chain(True)
        got = b.run().tolist()
        ci = b.chain_info()
    finally:
        b.close()
    assert ci["chain_pairs"] == npairs and ci["chain_jobs"] == per_pair * npairs >= 2 * resident and ci["chunks"] == 1
    want, _ = pa.Batch(pairs).run()  # the bit-packed kernel
    assert got == want.tolist()
    assert got == plain
    assert got[:8] == [ap.affine_nw(x, y, cm)[0] for x, y in pairs[:8]]


def test_budget(monkeypatch):
    rng = np.random.default_rng(51)
    letters = np.frombuffer(b"ACGT", np.uint8)

    def pair(n, m):
        y = letters[rng.integers(0, 4, m)]
        x = letters[rng.integers(0, 4, n)]
        x[:m] = np.where(rng.random(m) < 0.1, x[:m], y)  # a noisy copy of y, then a random tail
        return x.tobytes(), y.tobytes()

    cm = AffineCost.affine(4, 6, 2)
    pairs = [pair(20000, 4097) for _ in range(8)]  # 5 strips: 4 rows of 20 001 values, 640 KB
    b = AffineBatch(pairs, cm)
    try:
        plain = b.run().tolist()
        b.set_chain(True)
        one = b.run().tolist()
        assert b.chain_info()["chunks"] == 1 and b.chain_info()["bnd_bytes_max"] == 8 * 4 * 20001 * 8
        monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
        several = b.run().tolist()
        ci = b.chain_info()
    finally:
        b.close()
    assert ci["chunks"] >= 4 and ci["bnd_bytes_max"] <= 1 << 20 and ci["chain_jobs"] == 40
    assert several == one == plain
    big = [pairs[0], pair(40000, 4097)]  # 1.28 MB of rows
    b = AffineBatch(big, cm, chain=True)
    try:
        with pytest.raises(ValueError, match="pa_affine_batch_run: pair 1"):
            b.run()
        b.set_chain(False)
        got = b.run().tolist()
        monkeypatch.delenv("PA_AFFINE_TRACE_BUDGET_MB")
        b.set_chain(True)
        assert b.run().tolist() == got and got[0] == plain[0]
    finally:
        b.close()
