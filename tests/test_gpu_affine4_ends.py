"""The ends-free (semi-global) mode of the batched double-affine aligner (Affine4Batch.set_free_ends) against the plain DP of
tests/affine4_ends_plain.py: cost, start, end, exact CIGAR string and the whole last row of every pair, plus an independent pricing of
the CIGAR on a[start:end], through run(), align(), align_tiled() and the chained route, over the pairs of tests/affine4_ends_cases.py."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch
from tests import affine4_ends_cases as cases
from tests import affine4_plain as a4
from tests import affine_heavy_cases as heavy
from tests.affine4_ends_plain import affine4_ends

pytestmark = pytest.mark.gpu

R = cases.R
MODELS = cases.MODELS
_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def oracle(pairs, name, fs, fe):
    """(cost, start, end, cigar, last_row) of every pair; computed once per (pair, model, setting)."""
    out = []
    for x, y in pairs:
        key = (x, y, name, fs, fe)
        if key not in _ORACLE:
            _ORACLE[key] = affine4_ends(x, y, MODELS[name], fs, fe)
        out.append(_ORACLE[key])
    return out


def batch(pairs, name, fs=False, fe=False, trace=True, chain=False):
    b = Affine4Batch(pairs, MODELS[name], trace=trace, chain=chain)
    if fs or fe:
        b.set_free_ends(fs, fe)
    return b


def check_rows(b, pairs, want):
    rows = b.last_row()
    assert len(rows) == len(pairs)
    for p, (row, w) in enumerate(zip(rows, want)):
        assert row.dtype == np.int32 and row.tolist() == w[4].tolist(), (p, len(pairs[p][0]), len(pairs[p][1]))


def check_cost_only(b, pairs, want, fs):
    assert b.run().tolist() == [w[0] for w in want]
    assert b.ends().tolist() == [[-1 if fs else 0, w[2]] for w in want]


def check_traced(b, pairs, name, want, got):
    assert len(got) == len(pairs)
    ends = b.ends().tolist()
    for p, ((x, y), w, (c, g)) in enumerate(zip(pairs, want, got)):
        assert (c, ends[p][0], ends[p][1], g) == w[:4], (p, len(x), len(y))
        assert a4.affine4_verify(g, x[w[1]:w[2]], y, MODELS[name]) == c


def check_all_routes(pairs, name, fs, fe, tile_cols=64):
    want = oracle(pairs, name, fs, fe)
    b = batch(pairs, name, fs, fe)
    try:
        check_cost_only(b, pairs, want, fs)
        check_traced(b, pairs, name, want, b.align())
        check_traced(b, pairs, name, want, b.align_tiled(tile_cols))
        check_rows(b, pairs, want)
    finally:
        b.close()


@pytest.mark.parametrize("fs,fe", cases.SETTINGS, ids=[f"{int(fs)}{int(fe)}" for fs, fe in cases.SETTINGS])
def test_every_setting_at_the_shape_edges(fs, fe):
    """Every |b| of EDGE_M with every |a| of edge_n(|b|), 45 pairs in one batch."""
    check_all_routes(cases.edge_all(), "double_affine", fs, fe)


@pytest.mark.parametrize("name", ("asymmetric", "linear_edges"))
def test_the_other_models_with_both_ends_free(name):
    check_all_routes(cases.flanked() + cases.edge_pairs(len(name) % 5), name, True, True)


@pytest.mark.parametrize("fs,fe", [(True, True), (False, True)])
def test_packed_wavefront_with_unequal_texts(fs, fe):
    pairs = cases.packed_unequal()
    b = batch(pairs, "double_affine", trace=False)
    info = b.info()
    b.close()
    assert info["waves"] == 1 and info["packed_pairs"] == len(pairs) and len({len(x) for x, _ in pairs}) > len(pairs) // 2
    check_all_routes(pairs, "double_affine", fs, fe)


def test_tiled_route_at_the_tile_edges():
    name = "double_affine"
    pairs = cases.tile_edges() + cases.two_piece()
    want = oracle(pairs, name, True, True)
    b = batch(pairs, name, True, True)
    try:
        got = b.align_tiled(cases.TILE_COLS)
        check_traced(b, pairs, name, want, got)
        visits = sum(-(-len(x) // cases.TILE_COLS) + -(-max(len(y), 1) // (64 * R)) for x, y in pairs)  # tile_visits_max, summed
        assert 0 < b.tiled_info()["tile_jobs"] <= visits
        assert b.align() == got
        check_cost_only(b, pairs, want, True)
        check_rows(b, pairs, want)
        b.set_free_ends(True, False)
        check_traced(b, pairs, name, oracle(pairs, name, True, False), b.align_tiled(cases.TILE_COLS))
    finally:
        b.close()


@pytest.mark.parametrize("fs,fe", [(True, True), (False, True)])
def test_chained_route(fs, fe):
    name = "double_affine"
    pairs = [(x, y) for x, y in cases.edge_pairs(0) + cases.edge_pairs(1) if len(y) > 64 * R] + cases.flanked()[:4] + cases.two_piece()[1:2]
    assert {len(y) for _, y in pairs} >= {64 * R + 1, 128 * R + 77}
    want = oracle(pairs, name, fs, fe)
    b = batch(pairs, name, fs, fe)
    try:
        plain_costs, plain = b.run().tolist(), b.align_tiled(64)
        plain_ends = b.ends().tolist()
        b.set_chain(True)
        check_cost_only(b, pairs, want, fs)
        assert b.chain_info()["chain_pairs"] == sum(len(y) > 64 * R for _, y in pairs) > 0
        got = b.align_tiled(64)
        check_traced(b, pairs, name, want, got)
        assert b.chain_info()["chain_pairs"] > 0
        assert got == plain and b.ends().tolist() == plain_ends and [c for c, _ in got] == plain_costs
        check_rows(b, pairs, want)
    finally:
        b.close()
    b = batch(pairs, name, fs, fe, chain=True)  # chained from the start
    try:
        check_cost_only(b, pairs, want, fs)
    finally:
        b.close()


def test_setting_toggled_on_one_batch():
    name = "double_affine"
    pairs = cases.flanked() + cases.two_piece()
    fresh = batch(pairs, name)
    try:
        fresh_costs, fresh_align, fresh_tiled = fresh.run().tolist(), fresh.align(), fresh.align_tiled(64)
    finally:
        fresh.close()
    assert fresh_align == fresh_tiled == [a4.affine4_nw(x, y, MODELS[name]) for x, y in pairs]
    b = batch(pairs, name)
    try:
        with pytest.raises(ValueError, match="pa_affine4_batch_ends"):
            b.ends()  # before any run
        for fs, fe in ((False, False), (True, True), (False, True), (False, False)):
            b.set_free_ends(fs, fe)
            with pytest.raises(ValueError, match="pa_affine4_batch_ends"):
                b.ends()  # after a change of setting, without a run
            want = oracle(pairs, name, fs, fe)
            check_cost_only(b, pairs, want, fs)
            check_traced(b, pairs, name, want, b.align())
            if not (fs or fe):  # the global results are those of a batch that never left global mode
                assert b.run().tolist() == fresh_costs and b.align() == fresh_align and b.align_tiled(64) == fresh_tiled
                assert b.ends().tolist() == [[0, len(x)] for x, _ in pairs]
        b.set_free_ends(True, True)
        b.run()
        assert (b.ends()[:, 0] == -1).all()
        with pytest.raises(ValueError):
            b.set_free_ends(2, 0)
        assert (b.ends()[:, 0] == -1).all()  # a refused setting changes nothing
    finally:
        b.close()


def test_empty_batch():
    b = batch([], "double_affine", True, True)
    try:
        assert b.run().tolist() == [] and b.ends().shape == (0, 2)
        assert b.align() == [] and b.align_tiled() == [] and b.ends().shape == (0, 2) and b.last_row() == []
    finally:
        b.close()
    assert pa.map_affine([], MODELS["double_affine"]) == []


def test_last_row_in_global_mode_and_skipped_pairs():
    pairs = cases.flanked() + cases.edge_all()[-2:]
    want = oracle(pairs, "linear_edges", False, False)
    b = batch(pairs, "linear_edges", trace=False)
    try:
        costs = b.run().tolist()
        rows = b.last_row()
        assert [int(r[-1]) for r in rows] == costs == [w[0] for w in want]
        check_rows(b, pairs, want)
        some = [len(pairs) - 1, 3, 0, 17]
        got = b.last_row(some)
        assert len(got) == 4 and all(g.tolist() == rows[p].tolist() for g, p in zip(got, some))
        assert b.last_row([]) == []
        assert b.run().tolist() == costs  # the pass of last_row() leaves the batch as it was
        with pytest.raises(ValueError):
            b.last_row([0, 0])
    finally:
        b.close()


def test_last_row_budget(monkeypatch):
    rng = np.random.default_rng(71)
    y = cases.rand_seq(rng, 5)
    pairs = [(cases.rand_seq(rng, 100000 + 1000 * k), y) for k in range(4)] + cases.flanked()[:3]  # 400 KB of row each
    b = batch(pairs, "double_affine", False, True, trace=False)
    try:
        one = b.last_row()
        monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
        several = b.last_row()  # two of the long rows to a chunk
        assert all(s.tolist() == o.tolist() for s, o in zip(several, one))
        costs = b.run().tolist()
        assert costs == [int(r.min()) for r in one] and b.ends()[:, 1].tolist() == [int(np.argmin(r)) for r in one]
        assert [r.tolist() for r in one[4:]] == [w[4].tolist() for w in oracle(pairs[4:], "double_affine", False, True)]
    finally:
        b.close()
    big = [pairs[4], (b"AC" * 140000, y)]  # 1.12 MB of row
    b = batch(big, "double_affine", trace=False)
    try:
        with pytest.raises(ValueError, match="pa_affine4_batch_last_row: pair 1"):
            b.last_row()
        assert len(b.last_row([0])[0]) == len(big[0][0]) + 1  # without the pair that does not fit
    finally:
        b.close()


def test_any_byte_with_both_ends_free():
    check_all_routes(cases.any_byte(), "double_affine", True, True)


def test_map_affine_equals_the_batch_calls():
    pairs = cases.flanked()
    cm = MODELS["double_affine"]
    want = oracle(pairs, "double_affine", True, True)
    assert pa.map_affine(pairs, cm) == [(w[0], w[3], w[1], w[2]) for w in want]
    assert pa.map_affine(pairs, cm, tiled=True, chain=True) == pa.map_affine(pairs, cm)
    half = oracle(pairs, "double_affine", False, True)
    assert pa.map_affine(pairs, cm, free_start=False, tiled=True) == [(w[0], w[3], w[1], w[2]) for w in half]
    assert [(c, g) for c, g, _, _ in pa.map_affine(pairs, cm, free_start=False, free_end=False)] == pa.align_affine4(pairs, cm)


def heavy_expected(cm, N):
    """(cost, end) of heavy.thin_limit(cm, N) with both ends free, in closed form: an empty text leaves the pattern to one insertion
    and end = 0; the text C under a pattern of N - 1 bytes with one C is matched between two insertions (one insertion of all N - 1
    bytes pays an extend more than the second open) and end = 1; a pattern that is empty, or the one byte the text holds, costs 0 at
    the lowest column that can end it."""
    k = heavy.thin_k(N)
    wi = lambda L: heavy.gap_w(L, cm.ins, [(o, e) for kind, o, e in cm.layers if kind == "ins"])  # noqa: E731
    return [(0, 0), (wi(N), 0), (0, k + 1), (wi(k) + wi(N - 2 - k), 1)]


def test_costs_of_1000_and_a_total_near_2_30():
    """A model whose every cost is 999 or 1000 on the four thin pairs whose global totals are next to 2^30, both ends free.  The plain
    DP takes minutes on a million rows, so it is asked about the same four pairs at N = 300, where it must give the closed forms that
    the million-row pairs are then held to; the ends-free values are never above the global ones, which the check at creation bounds."""
    cm = heavy.THIN_MODELS4["four_1_999"]
    small = heavy.thin_limit(cm, 300)
    assert [(w[0], w[2]) for w in (affine4_ends(x, y, cm, True, True, trace=False) for x, y in small)] == heavy_expected(cm, 300)
    N = heavy.thin_n(cm)
    pairs, want = heavy.thin_limit(cm), heavy_expected(cm, N)
    glob = heavy.thin_expected(cm)
    assert all(heavy.LIMIT - heavy.LIMIT // 500 <= c < heavy.LIMIT for c, _ in glob) and all(w[0] <= g[0] for w, g in zip(want, glob))
    assert max(w[0] for w in want) >= heavy.LIMIT - heavy.LIMIT // 500  # one of them stays next to the bound with its ends free
    b = Affine4Batch(pairs, cm)
    try:
        b.set_free_ends(True, True)
        assert b.run().tolist() == [w[0] for w in want]
        assert b.ends().tolist() == [[-1, w[1]] for w in want]
        b.set_free_ends(False, False)
        assert b.run().tolist() == [c for c, _ in glob]
    finally:
        b.close()
