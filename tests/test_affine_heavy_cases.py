"""Are the pairs of tests/affine_heavy_cases.py worth running?  The plain oracles alone answer (no GPU): the DT pairs cost what the NW
oracle says and reach the costs at which the ring, the empty fronts, the affine reach and the segments of the diagonal-transition routes
are exercised; the gaps have the lengths at which the linear edge and the pieces take over from each other; the aimed runs of the strip
pairs are open at their edges; and the closed forms of the thin pairs next to 2^30 are those of the plain DP.  This is what keeps
tests/test_gpu_affine_heavy.py from passing for a dull reason.

Measured here: the whole file takes 50 to 55 s on 8 cores: 12 to 20 s for the plain DT of every DT pair under the six models (a module
fixture, spread over worker processes; 100 s in one), 18 s for the four-layer DT under the five models of MODELS4 with the ends-free
lists and the wide batch (the same way; 150 s in one), 9 s for the two segmented plain walks, 5 s for the count of empty fronts."""
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from tests import affine4_plain as a4
from tests import affine_heavy_cases as cases
from tests import affine_plain as ap
from tests.affine_dt_ends_plain import affine_dt_ends
from tests import affine_dt_plain as dtp
from tests.affine_dt_plain import affine_dt
from tests.affine_dt_seg_plain import affine_dt_seg, bound_of, max_edge, seg_of

MODELS, MODELS4 = cases.MODELS, cases.MODELS4
DT = cases.dt_cases()
BIG = (1 << 30) - 1
E = 1000


@pytest.fixture(scope="module")
def dt():
    """{model: {case: [(cost, CIGAR)]}} by the plain DT, once: 1.7 million cost steps, about 100 s in one process, so fresh worker
    processes take a (model, case) each (started, not forked: they share nothing with this process)."""
    keys = [(name, c) for name in MODELS for c in DT]
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as pool:
        res = list(pool.map(cases.dt_oracle_case, *zip(*keys)))
    cases.DT_ORACLE.update(zip(keys, res))  # kept for the other test modules of the session
    return {name: {c: cases.DT_ORACLE[name, c] for c in DT} for name in MODELS}


def costs_of(dt, name):
    return [c for res in dt[name].values() for c, _ in res]


def test_models_are_what_the_names_say():
    assert all(max_edge(cm) == E for cm in MODELS.values())
    assert sorted(MODELS) == ["cheap_sub", "coprime", "crossover", "flat_1000", "linear_heavy", "no_sub_heavy"]
    w = lambda cm, L: cases.gap_w(L, cm.ins, [(o, e) for k, o, e in cm.layers if k == "ins"])  # noqa: E731
    cross = MODELS["crossover"]
    assert [w(cross, L) for L in (1, 2, 3, 4)] == [700, 1400, 1900, 2200] and 3 * 700 > 1900 and 1000 + 2 * 300 > 1400
    dbl = MODELS4["double_heavy"]
    assert 100 + 3 * 700 == 1000 + 3 * 400 and 100 + 2 * 700 < 1000 + 2 * 400 and 100 + 4 * 700 > 1000 + 4 * 400 and w(dbl, 3) == 2200
    assert any(e == 1000 for _, _, e in MODELS4["asymmetric_heavy"].layers) and MODELS4["no_sub4_heavy"].sub is None
    for cm in list(MODELS.values()):
        cm.to_c()
    for cm in list(MODELS4.values()) + list(cases.THIN_MODELS4.values()):
        cm.to_c4()


def test_nw_and_dt_costs_agree(dt):
    for name, cm in MODELS.items():
        for c, pairs in DT.items():
            for (x, y), (cost, cigar) in zip(pairs, dt[name][c]):
                assert cost == ap.affine_nw(x, y, cm, trace=False)[0], (name, c, len(x), len(y))
                assert ap.affine_verify(cigar, x, y, cm) == cost
            assert all(len(x) <= 120 and len(y) <= 120 for x, y in pairs)


def test_costs_reach_the_mechanisms(dt):
    for name in MODELS:
        if name != "cheap_sub":
            assert max(costs_of(dt, name)) > 20 * E, name
    flat = costs_of(dt, "flat_1000")
    assert max(c for c, _ in dt["flat_1000"]["dt_gap"]) >= 20000 and all(c % 1000 == 0 for c in flat)
    assert 0 in flat and 1000 in flat and 2000 in flat                      # below, on and above E
    cheap = costs_of(dt, "cheap_sub")
    assert max(cheap) > 1001 and {1, 1001} <= set(cheap)                     # the ring wraps with live fronts, and the layer opens
    assert len({c % 1000 for c in costs_of(dt, "coprime")}) > 20             # many residues
    assert any(c < E for c in costs_of(dt, "cheap_sub")) and any(0 < c < E for c in costs_of(dt, "crossover"))


def front_is_empty(a, b, cm, cost, monkeypatch):
    """Per cost 0 .. `cost`: does the plain DT's front hold nothing on any layer?  Counted inside affine_dt itself: every front it
    stores (insert, delete and main layer of every cost, in that order) is looked at on its way into the store."""
    seen = []
    put = dtp._Fronts.put

    def spy(self, lo, arr):
        seen.append(bool((np.asarray(arr) >= 0).any()))
        put(self, lo, arr)

    monkeypatch.setattr(dtp._Fronts, "put", spy)
    assert affine_dt(a, b, cm, cost)[0] == cost
    monkeypatch.undo()
    assert len(seen) == 3 * (cost + 1)
    return [not any(seen[3 * s:3 * s + 3]) for s in range(cost + 1)]


def test_flat_1000_fronts_are_mostly_empty(dt, monkeypatch):
    """At least 99 % of the fronts 0 .. cost of the dt_gap pairs hold nothing: only multiples of 1000 are costs of anything."""
    cm = MODELS["flat_1000"]
    for (x, y), (cost, _) in zip(DT["dt_gap"], dt["flat_1000"]["dt_gap"]):
        empty = front_is_empty(x, y, cm, cost, monkeypatch)
        assert sum(empty) >= 0.99 * (cost + 1), (sum(empty), cost)
        assert not empty[0] and not empty[cost] and all(empty[s] for s in range(cost) if s % 1000)


SEG_MODELS = ("flat_1000", "coprime", "cheap_sub", "linear_heavy")
SEG_ODD = E + 337


def test_segments(dt):
    """The costs against the segment sizes, by the helpers of tests/affine_dt_seg_plain.py, at the bound the GPU test passes (the
    batch's largest cost) for the batch it passes (cases.SEG_CASES)."""
    for name in SEG_MODELS:
        cm = MODELS[name]
        pairs, want = seg_batch(dt, name)
        top = max(c for c, _ in want)
        nseg = {seg: [c // seg_of(bound_of(len(x), len(y), cm, top, False, False), E, seg) + 1 for (x, y), (c, _) in zip(pairs, want)]
                for seg in (E, 0, SEG_ODD)}
        if name != "cheap_sub":
            assert max(nseg[E]) >= 10, name
            assert max(nseg[0]) >= 3, name
        assert any(c < E for c, _ in want)
    # exact multiples of S, and one more: under flat_1000 at seg = E every cost is a multiple; cheap_sub's one inserted byte costs 1001
    flat = [c for c, _ in seg_batch(dt, "flat_1000")[1]]
    assert any(c and c % E == 0 for c in flat)
    cheap = [c for c, _ in seg_batch(dt, "cheap_sub")[1]]
    assert any(c > E and c % E == 1 for c in cheap)
    assert all(c % SEG_ODD for c in flat if c)  # SEG_ODD divides no cost, and E does not divide it


def seg_batch(dt, name):
    pairs = [p for c in cases.SEG_CASES for p in DT[c]]
    return pairs, [r for c in cases.SEG_CASES for r in dt[name][c]]


@pytest.mark.parametrize("name, which, seg", [("flat_1000", 0, E), ("coprime", 1, 0)])
def test_gap_walk_crosses_boundaries_in_a_layer(name, which, seg, dt):
    """The dt_gap walk is in a layer at two segment boundaries and more; the segmented plain walk gives the plain DT's result."""
    cm = MODELS[name]
    (x, y), (cost, cigar) = DT["dt_gap"][which], dt[name]["dt_gap"][which]
    c, st, en, g, rec = affine_dt_seg(x, y, cm, cost, seg)
    assert (c, st, en, g) == (cost, 0, len(x), cigar)
    assert sum(layer != 0 for layer in rec["crossed"]) >= 2, (name, seg, rec)
    assert rec["nseg"] == cost // rec["seg"] + 1 >= 3


def gap_lengths(cigar):
    return [k for k, op in ap.cigar_elems(cigar) if op in "ID"]


def test_crossover_gap_lengths(dt):
    cm = MODELS["crossover"]
    cigars = [g for res in dt["crossover"].values() for _, g in res]
    lens = [k for g in cigars for k in gap_lengths(g)]
    assert any(k <= 2 for k in lens) and any(k >= 4 for k in lens) and 3 in lens
    lin = cases.cut_layers(cm, 0)  # the layers cut off: the linear indel alone
    assert any(ap.affine_nw(x, y, lin, trace=False)[0] != c for c_, pairs in DT.items() for (x, y), (c, _) in zip(pairs, dt["crossover"][c_]))
    (x, y), (c, g) = DT["dt_runs"][0], dt["crossover"]["dt_runs"][0]
    assert (c, sorted(gap_lengths(g))) == (700 + 1400 + 1900 + 2200, [1, 2, 3, 4])


def four_pairs():
    return cases.dt_runs() + cases.dt_gap() + cases.dt_mutated()[:2]


def test_double_heavy_gap_lengths():
    cm = MODELS4["double_heavy"]
    pairs = four_pairs()
    res = [a4.affine4_nw(x, y, cm) for x, y in pairs]
    lens = [k for _, g in res for k in gap_lengths(g)]
    assert any(k <= 2 for k in lens) and any(k >= 4 for k in lens) and 3 in lens
    two = cases.cut_layers(cm, 2)
    assert any(ap.affine_nw(x, y, two, trace=False)[0] != c for (x, y), (c, _) in zip(pairs, res))
    assert res[0][0] == 800 + 1500 + 2200 + 2600 and sorted(gap_lengths(res[0][1])) == [1, 2, 3, 4]
    for (x, y), (c, g) in zip(pairs[:3], res):
        assert a4.general_gap_cost(x, y, cm) == c  # a DP without layers agrees


@pytest.mark.parametrize("name", sorted(MODELS))
def test_aimed_runs_are_open_at_their_edges(name):
    from astar_pairwise_aligner_amd.capi import AFFINE_ROWS_PER_LANE as R

    aimed = [(x, y, aim) for x, y, aim in cases.nw_edges_aimed(R) if aim]
    assert len(aimed) == 7 and {aim for _, _, aim in aimed} == {("I", 64 * R), ("D", 64)}
    for x, y, aim in aimed:
        assert cases.aim_is_met(ap.affine_nw(x, y, MODELS[name])[1], aim), (name, len(x), len(y), aim)


@pytest.mark.parametrize("name", sorted(MODELS4))
def test_aimed_runs_are_open_at_their_edges_four_layers(name):
    from astar_pairwise_aligner_amd.capi import AFFINE4_ROWS_PER_LANE as R

    for x, y, aim in cases.nw_edges_aimed(R):
        if aim:
            assert cases.aim_is_met(a4.affine4_nw(x, y, MODELS4[name])[1], aim), (name, len(x), len(y), aim)


def test_edge_shapes():
    from astar_pairwise_aligner_amd.capi import AFFINE_ROWS_PER_LANE as R

    all_ = cases.nw_edges_aimed(R)
    assert len(all_) == 21 and all((aim is not None) == (p % 3 == 2) for p, (_, _, aim) in enumerate(all_))
    shapes = [(len(x), len(y)) for x, y, aim in all_ if aim is None]
    assert {m for _, m in shapes} == set(cases.edge_m(R)) and {n for n, _ in shapes} == set(cases.EDGE_N)
    assert any(len(y) > 64 * R for x, y, aim in all_ if aim is None)


def thin_all():
    return [(name, cm, ap.affine_nw, ap.affine_verify) for name, cm in cases.THIN_MODELS.items()] + \
           [(name, cm, a4.affine4_nw, a4.affine4_verify) for name, cm in cases.THIN_MODELS4.items()]


@pytest.mark.parametrize("name, cm, nw, verify", thin_all(), ids=[t[0] for t in thin_all()])
def test_thin_limit(name, cm, nw, verify):
    N, edge = cases.thin_n(cm), cases.create_max_edge(cm)
    assert edge == cm.max_edge() == 1000
    assert (N + 1) * edge < cases.LIMIT <= (N + 2) * edge
    pairs, want = cases.thin_limit(cm), cases.thin_expected(cm)
    for (x, y), (cost, cigar) in zip(pairs, want):
        assert len(x) + len(y) == N
        assert cases.LIMIT - cases.LIMIT // 500 <= cost < cases.LIMIT, (name, cost)
        assert verify(cigar, x, y, cm) == cost
    # the same shapes at N = 2000: the closed forms are the plain DP's, cost and CIGAR
    small = cases.thin_limit(cm, 2000)
    assert [nw(x, y, cm) for x, y in small] == cases.thin_expected(cm, 2000)


def test_planted_pairs_for_the_ends_free_route():
    """Texts of at most 150 bytes; under flat_1000 some hit lies inside its text and costs several E."""
    pairs = cases.dt_planted()
    assert all(len(x) <= 150 for x, _ in pairs)
    res = [affine_dt_ends(x, y, MODELS["flat_1000"], BIG, True, True) for x, y in pairs]
    assert any(0 < st and en < len(x) and c > 2 * E for (x, _), (c, st, en, _) in zip(pairs, res))
    assert any(en == len(x) for (x, _), (c, st, en, _) in zip(pairs, res)) and any(st == 0 for c, st, en, _ in res)


# ---- the four-layer DT route at heavy costs

DT4 = cases.dt4_cases()
DENSE, MAIN_EDGE = "dense4", "main_edge4"


@pytest.fixture(scope="module")
def dt4():
    """{model: {case: [(cost, CIGAR)]}} by the plain four-layer DT, once, a (model, case) to a worker process like `dt` above
    (cases.fill_dt4_oracle); the ends-free lists and the wide batch of the GPU tests go along."""
    cases.fill_dt4_oracle()
    return {name: {c: cases.DT4_ORACLE[name, c] for c in DT4} for name in MODELS4}


def main_edge4(cm):
    """pa::affine4::dt main_edge restated: the largest edge at which the main layer is read (sub, ins, del and the four opens)."""
    return max([v for v in (cm.sub, cm.ins, cm.del_) if v is not None] + [o for _, o, _ in cm.layers])


def ring_depths(cm):
    """The five ring depths of a cost-only four-layer DT call (shape_of restated): main_edge + 1, and extend_t + 1 per layer."""
    return [main_edge4(cm) + 1] + [e + 1 for _, _, e in cm.layers]


def test_four_layer_models_are_what_the_names_say():
    assert sorted(MODELS4) == ["asymmetric_heavy", "dense4", "double_heavy", "main_edge4", "no_sub4_heavy"]
    dense, edge = MODELS4[DENSE], MODELS4[MAIN_EDGE]
    assert ring_depths(dense) == [1001, 2, 2, 3, 4] and dense.sub == 1 and dense.ins is None and dense.del_ is None
    assert min(o for _, o, _ in dense.layers) >= 998  # no layer opens before s = 998
    assert ring_depths(edge) == [1001, 1001, 521, 781, 301]
    assert main_edge4(edge) == edge.sub == E and max(o for _, o, _ in edge.layers) < 300 and max(e for _, _, e in edge.layers) == 1000
    assert (edge.ins, edge.del_) == (999, 998)
    # depths the first three models never give
    old = {d for name in ("double_heavy", "asymmetric_heavy", "no_sub4_heavy") for d in ring_depths(MODELS4[name])}
    assert not {2, 3, 4, 301, 521, 781} & old
    for name in (DENSE, MAIN_EDGE):
        MODELS4[name].to_c4()
    wi = lambda cm, L: cases.gap_w(L, cm.ins, [(o, e) for k, o, e in cm.layers if k == "ins"])  # noqa: E731
    wd = lambda cm, L: cases.gap_w(L, cm.del_, [(o, e) for k, o, e in cm.layers if k == "del"])  # noqa: E731
    assert wi(dense, 1) == wd(dense, 1) == 1001 == 999 + 2 == 998 + 3 and wi(dense, cases.GAP) == wd(dense, cases.GAP) == 1020
    assert [wi(edge, L) for L in (1, 2)] == [999, 299 + 1560] and [wd(edge, L) for L in (1, 2)] == [530, 299 + 600]


def test_four_layer_nw_and_dt_costs_agree(dt4):
    for name, cm in MODELS4.items():
        for c, pairs in DT4.items():
            assert len(dt4[name][c]) == len(pairs)
            for (x, y), (cost, cigar) in zip(pairs, dt4[name][c]):
                assert cost == a4.affine4_nw(x, y, cm, trace=False)[0], (name, c, len(x), len(y))
                assert a4.affine4_verify(cigar, x, y, cm) == cost
            assert all(len(x) <= 120 and len(y) <= 120 for x, y in pairs)
    far = DT4["dt_far"]
    assert [len(x) - len(y) for x, y in far] == [cases.FAR4, -cases.FAR4] and cases.FAR4 == 65 > 64
    assert len(DT4["dt_ladder"]) == 6
    for (x, y), (cost, cigar) in zip(cases.dt4_wide(), cases.DT4_ORACLE["wide"]):
        assert cost == a4.affine4_nw(x, y, MODELS4[DENSE], trace=False)[0] and a4.affine4_verify(cigar, x, y, MODELS4[DENSE]) == cost
    for name in cases.DT4_ENDS_MODELS:
        from tests.affine4_ends_plain import affine4_ends

        for fs in (False, True):
            for fe in (False, True):
                for (x, y), w in zip(cases.dt_planted(), cases.DT4_ORACLE[name, fs, fe]):
                    c, _, en, _, _ = affine4_ends(x, y, MODELS4[name], fs, fe, trace=False)
                    assert (c, en) == (w[0], w[3]), (name, fs, fe, len(x), len(y))
                    assert a4.affine4_verify(w[1], x[w[2]:w[3]], y, MODELS4[name]) == c


def test_four_layer_costs_reach_the_mechanisms(dt4):
    for name in MODELS4:
        costs = costs_of(dt4, name)
        if name != DENSE:  # (under the dense model a substitution costs 1 and nothing reaches 20 E)
            assert max(costs) > 20 * E, name
            assert any(0 < c < E for c in costs) or MODELS4[name].sub is None, name
        assert any(c > E for c in costs) and 0 in costs, name
    dense = costs_of(dt4, DENSE)
    assert {1, 1001} <= set(dense) and max(dense) > 1001  # the main ring wraps with live fronts, and the layers open
    assert [c for c, _ in dt4[DENSE]["dt_gap"]] == [1020, 1020]  # 1000 + 20: as derived
    edge = costs_of(dt4, MAIN_EDGE)
    assert any(c < E for c in edge) and E in edge and any(c > E for c in edge)  # below, on and above E
    assert 999 in edge and 530 in edge  # the linear insert, and layer 1, at length 1


def test_the_wide_batch_is_wide(dt4):
    from tests.affine4_dt_plain import mean_w

    want = cases.DT4_ORACLE["wide"]
    top = max(c for c, _ in want)
    assert mean_w(cases.dt4_wide(), MODELS4[DENSE], top) > 256 and top > 1130
    assert len({c for c, _ in want}) >= 3
