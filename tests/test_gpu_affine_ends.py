"""The ends-free (semi-global) mode of the batched gap-affine aligner (AffineBatch.set_free_ends) against the plain DP of
tests/affine_ends_plain.py: cost, start, end, exact CIGAR string and the whole last row of every pair, plus an independent pricing of the
CIGAR on a[start:end], through run(), align(), align_tiled() and the chained route, over the pairs of tests/affine_ends_cases.py."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch
from tests import affine_ends_cases as cases
from tests import affine_plain as ap
from tests.affine_ends_plain import affine_ends

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
            _ORACLE[key] = affine_ends(x, y, MODELS[name], fs, fe)
        out.append(_ORACLE[key])
    return out


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
        assert ap.affine_verify(g, x[w[1]:w[2]], y, MODELS[name]) == c
        assert ap.no_adjacent_same_op(g)


def check_all_routes(pairs, name, fs, fe, tile_cols=64):
    want = oracle(pairs, name, fs, fe)
    b = AffineBatch(pairs, MODELS[name], trace=True, free_start=fs, free_end=fe)
    try:
        check_cost_only(b, pairs, want, fs)
        check_traced(b, pairs, name, want, b.align())
        check_traced(b, pairs, name, want, b.align_tiled(tile_cols))
        check_rows(b, pairs, want)
    finally:
        b.close()


SETTING_CASES = [(name, fs, fe) for name in cases.SETTING_MODELS for fs, fe in cases.SETTINGS]


@pytest.mark.parametrize("name,fs,fe", SETTING_CASES, ids=[f"{n}-{int(fs)}{int(fe)}" for n, fs, fe in SETTING_CASES])
def test_every_setting_at_the_shape_edges(name, fs, fe):
    """Every |b| of EDGE_M with every |a| of edge_n(|b|), 45 pairs in one batch."""
    check_all_routes(cases.edge_all(), name, fs, fe)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_constructor_with_both_ends_free(name):
    pairs = cases.flanked()
    if name not in cases.SETTING_MODELS:  # (the others met the edge shapes above)
        pairs = pairs + cases.edge_pairs(len(name) % 5)
    check_all_routes(pairs, name, True, True)


@pytest.mark.parametrize("fs,fe", [(True, True), (False, True)])
def test_packed_wavefront_with_unequal_texts(fs, fe):
    pairs = cases.packed_unequal()
    b = AffineBatch(pairs, MODELS["affine"])
    info = b.info()
    b.close()
    assert info["waves"] == 1 and info["packed_pairs"] == len(pairs) and len({len(x) for x, _ in pairs}) > len(pairs) // 2
    check_all_routes(pairs, "affine", fs, fe)


@pytest.mark.parametrize("name", ("affine", "linear_affine"))
def test_tiled_route_at_the_tile_edges(name):
    pairs = cases.tile_edges()
    want = oracle(pairs, name, True, True)
    b = AffineBatch(pairs, MODELS[name], trace=True, free_start=True, free_end=True)
    try:
        got = b.align_tiled(cases.TILE_COLS)
        check_traced(b, pairs, name, want, got)
        visits = sum(-(-len(x) // cases.TILE_COLS) + -(-max(len(y), 1) // (64 * R)) for x, y in pairs)  # tile_visits_max, summed
        assert 0 < b.tiled_info()["tile_jobs"] <= visits
        assert b.align() == got
        b.set_free_ends(True, False)
        check_traced(b, pairs, name, oracle(pairs, name, True, False), b.align_tiled(cases.TILE_COLS))
    finally:
        b.close()


@pytest.mark.parametrize("fs,fe", [(True, True), (False, True), (True, False)])
def test_chained_route(fs, fe):
    pairs = [(x, y) for x, y in cases.edge_pairs(0) + cases.edge_pairs(1) if len(y) > 64 * R] + cases.flanked()[:4]
    assert {len(y) for _, y in pairs} >= {64 * R + 1, 128 * R + 77}
    want = oracle(pairs, "affine", fs, fe)
    b = AffineBatch(pairs, MODELS["affine"], trace=True, free_start=fs, free_end=fe)
    try:
        plain_costs, plain = b.run().tolist(), b.align_tiled(64)
        plain_ends = b.ends().tolist()
        b.set_chain(True)
        check_cost_only(b, pairs, want, fs)
        assert b.chain_info()["chain_pairs"] == sum(len(y) > 64 * R for _, y in pairs) > 0
        got = b.align_tiled(64)
        check_traced(b, pairs, "affine", want, got)
        assert b.chain_info()["chain_pairs"] > 0
        assert got == plain and b.ends().tolist() == plain_ends and [c for c, _ in got] == plain_costs
        check_rows(b, pairs, want)
    finally:
        b.close()


def test_setting_toggled_on_one_batch():
    pairs = cases.flanked()
    b = AffineBatch(pairs, MODELS["affine"], trace=True)
    try:
        with pytest.raises(ValueError, match="pa_affine_batch_ends"):
            b.ends()  # before any run
        for fs, fe in ((False, False), (True, True), (False, False), (False, True), (True, False)):
            b.set_free_ends(fs, fe)
            with pytest.raises(ValueError, match="pa_affine_batch_ends"):
                b.ends()  # after a change of setting, without a run
            want = oracle(pairs, "affine", fs, fe)
            check_cost_only(b, pairs, want, fs)
            check_traced(b, pairs, "affine", want, b.align())
            if not (fs or fe):
                assert b.align() == [ap.affine_nw(x, y, MODELS["affine"]) for x, y in pairs]
        b.set_free_ends(True, True)
        b.run()
        assert (b.ends()[:, 0] == -1).all()
        with pytest.raises(ValueError):
            b.set_free_ends(2, 0)
        assert (b.ends()[:, 0] == -1).all()  # a refused setting changes nothing
    finally:
        b.close()


def test_empty_batch():
    b = AffineBatch([], MODELS["affine"], trace=True, free_start=True, free_end=True)
    try:
        assert b.run().tolist() == [] and b.ends().shape == (0, 2)
        assert b.align() == [] and b.align_tiled() == [] and b.ends().shape == (0, 2) and b.last_row() == []
    finally:
        b.close()
    assert pa.map_affine([], MODELS["affine"]) == []


def test_last_row_in_global_mode_and_skipped_pairs():
    pairs = cases.flanked() + cases.edge_all()[-2:]
    want = oracle(pairs, "linear_affine", False, False)
    b = AffineBatch(pairs, MODELS["linear_affine"])
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
    b = AffineBatch(pairs, MODELS["unit"], free_end=True)
    try:
        one = b.last_row()
        monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
        several = b.last_row()  # two of the long rows to a chunk
        assert all(s.tolist() == o.tolist() for s, o in zip(several, one))
        costs = b.run().tolist()
        assert costs == [int(r.min()) for r in one] and b.ends()[:, 1].tolist() == [int(np.argmin(r)) for r in one]
        assert [r.tolist() for r in one[4:]] == [w[4].tolist() for w in oracle(pairs[4:], "unit", False, True)]
    finally:
        b.close()
    big = [pairs[4], (b"AC" * 140000, y)]  # 1.12 MB of row
    b = AffineBatch(big, MODELS["unit"])
    try:
        with pytest.raises(ValueError, match="pa_affine_batch_last_row: pair 1"):
            b.last_row()
        assert len(b.last_row([0])[0]) == len(big[0][0]) + 1  # without the pair that does not fit
    finally:
        b.close()


def test_any_byte_with_both_ends_free():
    for name in ("affine", "unit", "lcs"):
        check_all_routes(cases.any_byte(), name, True, True)


def test_map_affine_equals_the_batch_calls():
    pairs = cases.flanked()
    cm = MODELS["affine"]
    want = oracle(pairs, "affine", True, True)
    assert pa.map_affine(pairs, cm) == [(w[0], w[3], w[1], w[2]) for w in want]
    assert pa.map_affine(pairs, cm, tiled=True, chain=True) == pa.map_affine(pairs, cm)
    half = oracle(pairs, "affine", False, True)
    assert pa.map_affine(pairs, cm, free_start=False, tiled=True) == [(w[0], w[3], w[1], w[2]) for w in half]
    assert [(c, g) for c, g, _, _ in pa.map_affine(pairs, cm, free_start=False, free_end=False)] == pa.align_affine(pairs, cm)
