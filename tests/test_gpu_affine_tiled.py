"""The tiled gap-affine traceback (pa_affine_batch_align_tiled) against the plain DP of tests/affine_plain.py and against the untiled route:
cost and exact CIGAR string of every pair at the tile edges (rows at 1024, columns at tile_cols), gaps that cross an edge in their layer,
the border row and column, a mixed batch, the memory budget, and the tile accounting derived from the oracle's paths."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost
from tests import affine_plain as ap
from tests import affine_tiles_plain as tiles
from tests.test_gpu_affine import MODELS, mixed, mutate, rand_seq

pytestmark = pytest.mark.gpu

TILE_COLS = (64, 256, 1024)
GAP_MODELS = (AffineCost.affine(4, 6, 2), AffineCost.linear_affine(3, 2, 4, 1))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def check_tiled(pairs, cm, tile_cols=TILE_COLS, untiled=True):
    """align_tiled(C) of one batch for every C: the oracle's cost and CIGAR, the CIGAR priced on its own, align() of the same batch, and
    the tile accounting (one chunk at the default budget): tile jobs = the distinct tiles of the oracle's paths."""
    want = [ap.affine_nw(x, y, cm) for x, y in pairs]
    for (x, y), (c, g) in zip(pairs, want):
        assert ap.affine_verify(g, x, y, cm) == c
    b = AffineBatch(pairs, cm, trace=True)
    try:
        if untiled:
            assert b.align() == want
        for C in tile_cols:
            got = b.align_tiled(C)
            for p, (w, r) in enumerate(zip(want, got)):
                assert r == w, (C, p, len(pairs[p][0]), len(pairs[p][1]))
            per_pair = [len(tiles.path_tiles(g, C)) for _, g in want]
            info = b.tiled_info()
            assert info["chunks"] == (1 if pairs else 0)
            assert info["tile_jobs"] == sum(t for t, (x, y) in zip(per_pair, pairs) if x or y), (C, info, per_pair)
            assert info["refill_cells"] <= info["tile_jobs"] * (C + 1) * tiles.TILE_ROWS
            assert info["rounds"] <= max(per_pair, default=0)
            for t, (x, y) in zip(per_pair, pairs):
                assert t <= tiles.tiles_bound(len(x), len(y), C)
        assert b.run().tolist() == [c for c, _ in want]
    finally:
        b.close()
    return want


EDGE_M = (1023, 1024, 1025, 2048, 2049, 3000)


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
    check_tiled(edge_pairs(C, rotations, C), AffineCost.affine(4, 6, 2), tile_cols=(C,))


def test_identical_sequences_cross_tile_corners():
    y = rand_seq(np.random.default_rng(3), 2048)
    want = check_tiled([(y, y)], AffineCost.affine(4, 6, 2), tile_cols=(1024,))
    assert want == [(0, "2048=")]
    assert tiles.path_tiles(want[0][1], 1024) == [(0, 0), (1, 1)]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_constructor_at_reduced_edges(name):
    rng = np.random.default_rng(len(name))
    pairs = []
    for n, m in ((63, 1023), (64, 1024), (65, 1025), (129, 2049), (128, 700), (1100, 40)):
        y = rand_seq(rng, m)
        pairs.append(((mutate(rng, y, 0.1) + rand_seq(rng, n))[:n], y))
    check_tiled(pairs, MODELS[name], tile_cols=(64,))


def runs_of(cigar, op):
    """[(first state, last state)] of every run of `op` in the path."""
    out, i, j = [], 0, 0
    for k, o in ap.cigar_elems(cigar):
        di, dj = (k, k) if o in "=X" else (0, k) if o == "I" else (k, 0)
        if o == op:
            out.append(((i, j), (i + di, j + dj)))
        i, j = i + di, j + dj
    return out


@pytest.mark.parametrize("cm", GAP_MODELS, ids=("affine", "linear_affine"))
def test_insertion_run_across_row_1024(cm):
    rng = np.random.default_rng(21)
    y = rand_seq(rng, 2200)
    pairs = [(y, y[:1000] + rand_seq(rng, 60) + y[1000:])]
    _, g = ap.affine_nw(*pairs[0], cm)
    assert any(j0 < 1024 < j1 and j1 - j0 >= 50 for (_, j0), (_, j1) in runs_of(g, "I")), g  # the run is open in its layer at the edge
    check_tiled(pairs, cm)


@pytest.mark.parametrize("cm", GAP_MODELS, ids=("affine", "linear_affine"))
@pytest.mark.parametrize("C", TILE_COLS)
def test_deletion_run_across_column_C(C, cm):
    rng = np.random.default_rng(22 + C)
    y = rand_seq(rng, C + 300)
    pairs = [(y[: C - 25] + rand_seq(rng, 60) + y[C - 25:], y)]
    _, g = ap.affine_nw(*pairs[0], cm)
    assert any(i0 < C < i1 and i1 - i0 >= 50 for (i0, _), (i1, _) in runs_of(g, "D")), g
    check_tiled(pairs, cm, tile_cols=(C,))


def test_borders():
    rng = np.random.default_rng(23)
    pairs = [(b"", rand_seq(rng, 3000)), (rand_seq(rng, 3000), b""), (rand_seq(rng, 5), rand_seq(rng, 2500)),
             (rand_seq(rng, 2500), rand_seq(rng, 5)), (b"", b"")]
    for cm in GAP_MODELS:
        want = check_tiled(pairs, cm)
        assert tiles.path_tiles(want[0][1], 64) == [(0, 0), (0, 1), (0, 2)]
        assert len(tiles.path_tiles(want[1][1], 64)) == 47


def test_mixed_batch_shuffled_twice():
    cm = AffineCost.affine(4, 6, 2)
    pairs = mixed(7)
    b = AffineBatch(pairs, cm, trace=True)
    base = b.align()
    assert b.align_tiled(256) == base
    assert b.align_tiled(256) == base
    assert b.run().tolist() == [c for c, _ in base]
    b.close()
    perm = np.random.default_rng(8).permutation(len(pairs))
    b = AffineBatch([pairs[i] for i in perm], cm, trace=True)
    assert b.align_tiled(256) == [base[i] for i in perm]
    b.close()


def test_budget_that_refuses_the_untiled_route(monkeypatch):
    rng = np.random.default_rng(24)
    cm = AffineCost.affine(4, 6, 2)
    y = rand_seq(rng, 3000)
    pairs = [(b"ACGT" * 10, b"ACGT" * 10), ((mutate(rng, y, 0.05) + rand_seq(rng, 300))[:3000], y)]
    want = [ap.affine_nw(x, y, cm) for x, y in pairs]
    b = AffineBatch(pairs, cm, trace=True)
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
    with pytest.raises(ValueError, match="pair 1"):
        b.align()
    assert b.align_tiled(256) == want
    info = b.tiled_info()
    # row checkpoints 2 x 3001 x 8, column checkpoints 11 x 3073 x 8, a tile of 257 x 1025, 6000 ops (and the small pair's tile)
    assert 2 * 3001 * 8 + 11 * 3073 * 8 + 257 * 1025 + 6000 <= info["chunk_bytes_max"] <= 1 << 20
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "0.25")  # not even the tile
    with pytest.raises(ValueError, match="pair 1"):
        b.align_tiled(256)
    b.close()


def test_budget_chunks_give_the_same_result(monkeypatch):
    cm = AffineCost.linear_affine(3, 2, 4, 1)
    pairs = mixed(10)[:40]
    b = AffineBatch(pairs, cm, trace=True)
    one = b.align_tiled(256)
    assert one == b.align() and b.tiled_info()["chunks"] == 1
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")  # the largest pairs (2500 rows) need 0.5 MB each
    several = b.align_tiled(256)
    info = b.tiled_info()
    b.close()
    assert several == one
    assert info["chunks"] >= 4 and info["chunk_bytes_max"] <= 1 << 20


def test_rejected_arguments():
    b = AffineBatch([(b"ACGT" * 30, b"ACGT" * 30)], AffineCost.unit(), trace=True)
    for bad in (1, 63, (1 << 20) + 1):
        with pytest.raises(ValueError):
            b.align_tiled(bad)
    assert b.align_tiled(64) == b.align_tiled(1 << 20) == b.align_tiled() == [(0, "120=")]
    b.close()
    b = AffineBatch([(b"ACGT", b"ACGT")], AffineCost.unit())
    with pytest.raises(ValueError):  # created without trace
        b.align_tiled()
    b.close()


def test_align_affine_tiled():
    pairs = [(b"ACGTTGCA", b"ACGTGCA"), (b"", b"AC"), (b"AC", b"")]
    cm = AffineCost.affine(4, 6, 2)
    assert pa.align_affine(pairs, cm, tiled=True) == pa.align_affine(pairs, cm) == [ap.affine_nw(x, y, cm) for x, y in pairs]
