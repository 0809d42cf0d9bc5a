"""The tiled double-affine traceback (pa_affine4_batch_align_tiled) against the untiled route of the same batch and the plain DP of
tests/affine4_plain.py: cost and exact CIGAR string of every pair at the tile edges (rows at S = 64 R, columns at tile_cols), gaps of
both pieces that are open in their layer at an edge, the border row and column, every model, a mixed batch, the memory budget, and the
tile accounting derived from the paths."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineCost, capi
from tests import affine4_plain as a4
from tests import affine_tiles_plain as tiles
from tests.test_gpu_affine4 import DOUBLE, MODELS, mixed, mutate, rand_seq

pytestmark = pytest.mark.gpu

R = capi.AFFINE4_ROWS_PER_LANE
S = 64 * R  # rows of a row tile: one strip
assert S == tiles.TILE_ROWS  # tests/affine_tiles_plain.py has the two-layer route's geometry, which is this one at R = 16
TILE_COLS = (64, 256, 1024)
ORACLE_MAX = 1400  # affine4_nw takes about 0.5 s on 1300 x 1300


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def rows_of(m):
    if m > S:
        return -(-m // S) * S
    g = 1
    while g * R < m:
        g *= 2
    return g * R


def tiled_bytes(n, m, C):
    """Device bytes of one pair, as include/pa_affine4_tiled_hip.h states them."""
    H, r16 = rows_of(m), lambda x: (x + 15) & ~15
    strips = max(1, -(-m // S))
    return (strips - 1) * (n + 1) * 16 + r16(((n - 1) // C if n else 0) * (H + 1) * 12) + r16((min(n, C) + 1) * (min(H, S) + 1)) + n + m


def check_tiled(pairs, cm, tile_cols=TILE_COLS):
    """align_tiled(C) of one batch for every C against align() of the same batch, byte for byte; against the oracle's cost and CIGAR on
    the pairs it can take; the CIGAR priced on its own; and the tile accounting (one chunk at the default budget): tile jobs = the
    distinct tiles of the paths."""
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        base = b.align()
        for (x, y), (c, g) in zip(pairs, base):
            if max(len(x), len(y)) <= ORACLE_MAX:
                assert (c, g) == a4.affine4_nw(x, y, cm), (len(x), len(y))
            assert a4.affine4_verify(g, x, y, cm) == c
        for C in tile_cols:
            got = b.align_tiled(C)
            for p, (w, r) in enumerate(zip(base, got)):
                assert r == w, (C, p, len(pairs[p][0]), len(pairs[p][1]))
            per_pair = [len(tiles.path_tiles(g, C)) for _, g in base]
            info = b.tiled_info()
            assert info["chunks"] == (1 if pairs else 0)
            assert info["tile_jobs"] == sum(t for t, (x, y) in zip(per_pair, pairs) if x or y), (C, info, per_pair)
            assert info["refill_cells"] <= info["tile_jobs"] * (C + 1) * S
            assert info["rounds"] <= max(per_pair, default=0)
            assert info["chunk_bytes_max"] == sum(tiled_bytes(len(x), len(y), C) for x, y in pairs)
            for t, (x, y) in zip(per_pair, pairs):
                assert t <= tiles.tiles_bound(len(x), len(y), C)
        assert b.run().tolist() == [c for c, _ in base]
    finally:
        b.close()
    return base


EDGE_M = (S - 1, S, S + 1, 2 * S, 2 * S + 1, 3000)


def edge_n(C):
    return (C - 1, C, C + 1, 2 * C, 2 * C + 1)


def edge_pairs(C, rotations, seed):
    """|b| at the strip edges against |a| around C and 2C; rotation k pairs EDGE_M[q] with edge_n(C)[(q + k) % 5]."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in rotations:
        for q, m in enumerate(EDGE_M):
            y = rand_seq(rng, m)
            n = edge_n(C)[(q + k) % 5]
            x = mutate(rng, y, 0.1)
            x = (x + rand_seq(rng, max(n - len(x), 0)))[:n] if q % 2 else rand_seq(rng, n)
            assert len(x) == n
            pairs.append((x, y))
    return pairs


# every |b| meets every |a| of its C once or twice, not all of them: the oracle takes 0.2 s and more per pair
@pytest.mark.parametrize("C, rotations", [(64, (0, 1, 2)), (256, (0, 2)), (1024, (0,))])
def test_tile_edges(C, rotations):
    check_tiled(edge_pairs(C, rotations, C), DOUBLE, tile_cols=(C,))


def test_packed_pairs_of_every_width_class():
    rng = np.random.default_rng(17)
    pairs = []
    for lg in range(7):  # segments of g = 1 .. 64 lanes; three pairs per width, so that wavefronts hold several jobs
        for m, n in (((R << lg) - 3, 63), (R << lg, 130), (max((R << lg) - R + 1, 1), 200)):
            y = rand_seq(rng, m)
            pairs.append(((mutate(rng, y, 0.1) + rand_seq(rng, n))[:n], y))
    order = rng.permutation(len(pairs))
    check_tiled([pairs[k] for k in order], DOUBLE, tile_cols=(64, 256))


def test_identical_sequences_cross_tile_corners():
    y = rand_seq(np.random.default_rng(3), 2 * S)
    base = check_tiled([(y, y)], DOUBLE, tile_cols=(S,))
    assert base == [(0, f"{2 * S}=")]
    assert tiles.path_tiles(base[0][1], S) == [(0, 0), (1, 1)]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_model_at_reduced_edges(name):
    rng = np.random.default_rng(len(name))
    pairs = []
    for n, m in ((63, S - 1), (64, S), (65, S + 1), (129, 2 * S + 1), (128, 700), (1100, 40)):
        y = rand_seq(rng, m)
        pairs.append(((mutate(rng, y, 0.1) + rand_seq(rng, n))[:n], y))
    check_tiled(pairs, MODELS[name], tile_cols=(64,))


def runs_of(cigar, op):
    """[(first state, last state)] of every run of `op` in the path."""
    out, i, j = [], 0, 0
    for k, o in a4.cigar_elems(cigar):
        di, dj = (k, k) if o in "=X" else (0, k) if o == "I" else (k, 0)
        if o == op:
            out.append(((i, j), (i + di, j + dj)))
        i, j = i + di, j + dj
    return out


# Under double_affine(4, 6, 2, 24, 1) a gap of 12 lies in layer 0 / 1 (30 against 36), a gap of 60 in layer 2 / 3 (84 against 126).  The
# gap's bytes match nothing, so the gap has one best place.
@pytest.mark.parametrize("L", (12, 60))
def test_insertion_run_open_at_row_S(L):
    rng = np.random.default_rng(21 + L)
    y = rand_seq(rng, 1300)
    pairs = [(y, y[:S - L // 2] + rand_seq(rng, L, b"NRYK") + y[S - L // 2:])]
    c, g = a4.affine4_nw(*pairs[0], DOUBLE)
    assert c == (30 if L == 12 else 84)
    assert runs_of(g, "I") == [((S - L // 2, S - L // 2), (S - L // 2, S + L // 2))], g  # the run is open in its layer at row S
    assert check_tiled(pairs, DOUBLE) == [(c, g)]


@pytest.mark.parametrize("L", (12, 60))
def test_deletion_run_open_at_column_64(L):
    rng = np.random.default_rng(22 + L)
    y = rand_seq(rng, 264)
    pairs = [(y[:64 - L // 2] + rand_seq(rng, L, b"NRYK") + y[64 - L // 2:], y)]
    c, g = a4.affine4_nw(*pairs[0], DOUBLE)
    assert c == (30 if L == 12 else 84)
    assert runs_of(g, "D") == [((64 - L // 2, 64 - L // 2), (64 + L // 2, 64 - L // 2))], g
    assert check_tiled(pairs, DOUBLE, tile_cols=(64,)) == [(c, g)]


def test_borders():
    rng = np.random.default_rng(23)
    pairs = [(b"", rand_seq(rng, 3000)), (rand_seq(rng, 3000), b""), (rand_seq(rng, 5), rand_seq(rng, 2500)),
             (rand_seq(rng, 2500), rand_seq(rng, 5)), (b"", b"")]
    base = check_tiled(pairs, DOUBLE)
    for (x, y), got in zip(pairs, base):
        assert got == a4.affine4_nw(x, y, DOUBLE)  # (thin matrices: the oracle takes them whatever their length)
    assert tiles.path_tiles(base[0][1], 64) == [(0, 0), (0, 1), (0, 2)]
    assert len(tiles.path_tiles(base[1][1], 64)) == 47


def test_mixed_batch_shuffled_twice():
    pairs = mixed(7)
    b = Affine4Batch(pairs, DOUBLE, trace=True)
    base = b.align()
    assert b.align_tiled(256) == base
    assert b.align_tiled(256) == base
    assert b.run().tolist() == [c for c, _ in base]
    assert b.align() == base and b.info()["trace_chunks"] == 1
    b.close()
    perm = np.random.default_rng(8).permutation(len(pairs))
    b = Affine4Batch([pairs[i] for i in perm], DOUBLE, trace=True)
    assert b.align_tiled(256) == [base[i] for i in perm]
    assert b.last_forward_ms > 0 and b.last_refill_ms > 0 and b.last_walk_ms > 0
    b.close()


def test_budget_that_refuses_the_untiled_route(monkeypatch):
    rng = np.random.default_rng(24)
    y = rand_seq(rng, 3000)
    pairs = [(b"ACGT" * 10, b"ACGT" * 10), ((mutate(rng, y, 0.05) + rand_seq(rng, 300))[:3000], y)]
    b = Affine4Batch(pairs, DOUBLE, trace=True)
    base = b.align()
    for (x, y), (c, g) in zip(pairs, base):
        assert a4.affine4_verify(g, x, y, DOUBLE) == c
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
    with pytest.raises(ValueError, match="pair 1"):
        b.align()
    assert b.align_tiled(256) == base
    info = b.tiled_info()
    # row checkpoints 2 x 3001 x 16, column checkpoints 11 x 3073 x 12, a tile of 257 x 1025, 6000 ops (and the small pair's tile)
    assert tiled_bytes(3000, 3000, 256) >= 2 * 3001 * 16 + 11 * 3073 * 12 + 257 * 1025 + 6000
    assert tiled_bytes(3000, 3000, 256) <= info["chunk_bytes_max"] <= 1 << 20 and info["chunks"] == 1
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "0.25")  # not even the tile
    with pytest.raises(ValueError, match="pair 1"):
        b.align_tiled(256)
    b.close()


def test_budget_chunks_give_the_same_result(monkeypatch):
    pairs = mixed(10)[:40]
    b = Affine4Batch(pairs, MODELS["linear_edges"], trace=True)
    one = b.align_tiled(256)
    assert one == b.align() and b.tiled_info()["chunks"] == 1
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")  # the largest pairs (2500 rows) need 0.7 MB each
    several = b.align_tiled(256)
    info = b.tiled_info()
    b.close()
    assert several == one
    assert info["chunks"] >= 4 and info["chunk_bytes_max"] <= 1 << 20


def test_rejected_arguments():
    b = Affine4Batch([(b"ACGT" * 30, b"ACGT" * 30)], DOUBLE, trace=True)
    for bad in (1, 63, (1 << 20) + 1):
        with pytest.raises(ValueError, match="tile_cols"):
            b.align_tiled(bad)
    assert b.align_tiled(64) == b.align_tiled(1 << 20) == b.align_tiled() == [(0, "120=")]
    b.close()
    b = Affine4Batch([(b"ACGT", b"ACGT")], DOUBLE)
    with pytest.raises(ValueError, match="without trace"):  # created without trace
        b.align_tiled()
    b.close()


def test_align_affine4_tiled():
    pairs = [(b"ACGTTGCA", b"ACGTGCA"), (b"", b"AC"), (b"AC", b"")]
    assert pa.align_affine4(pairs, DOUBLE, tiled=True) == pa.align_affine4(pairs, DOUBLE) == [a4.affine4_nw(x, y, DOUBLE) for x, y in pairs]
