"""Every gap-affine route of both batch types under the seeded random cost models of tests/affine_random_cases.py
(tests/test_affine_random_cases.py says, without a GPU, why they are worth running): run, align, align_tiled, the four ends-free
settings on each of those, run_dt / align_dt at every bound of bounds_of, run_dt_ends / align_dt_ends, align_dt_seg on two layers, the
chained strips on two pairs of 1030 and 2060 rows, and map_affine / map_affine_dt on one model per class.  One test per model, so that a
failure names it; every comparison is exact, integers and CIGAR strings against the plain oracles, and every message carries the model.

A session that has run tests/test_affine_random_cases.py before finds the oracles' results in affine_random_cases.ORACLE; on its own
this module computes them first, a model to a worker process."""
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch
from tests import affine4_plain as a4
from tests import affine_plain as ap
from tests import affine_random_cases as cases
from tests.affine_dt_seg_plain import max_edge
from tests.affine_ends_cases import SETTINGS
from tests.test_gpu_affine4_dt import NOT_FOUND
from tests.test_gpu_affine4_dt import bounded as bounded4
from tests.test_gpu_affine_dt import bounded, bounds_of
from tests.test_gpu_affine_dt_seg import check_info

pytestmark = pytest.mark.gpu

M2, M4 = cases.models2(), cases.models4()
ALL = [(2, n) for n in M2] + [(4, n) for n in M4]
ONE_PER_CLASS = [(kind, next(n for n in ms if cases.class_of(n) == cls)) for kind, ms, classes in
                 ((2, M2, cases.TWO_CLASSES), (4, M4, cases.FOUR_CLASSES)) for cls in classes]


@pytest.fixture(scope="module", autouse=True)
def oracle():
    pa.require_gpu()
    return cases.fill_oracle(16)


def batch_of(kind):
    return Affine4Batch if kind == 4 else AffineBatch


def verify_of(kind):
    return a4.affine4_verify if kind == 4 else ap.affine_verify


def check_traced(pairs, cm, want, got, verify, what):
    """[(cost, CIGAR)] against the oracle's, pair by pair, each CIGAR priced on its own."""
    assert len(got) == len(pairs), (repr(cm), what)
    for p, ((x, y), w, g) in enumerate(zip(pairs, want, got)):
        assert g == w, (repr(cm), what, p, len(x), len(y))
        assert verify(g[1], x, y, cm) == g[0] and ap.no_adjacent_same_op(g[1]), (repr(cm), what, p, len(x), len(y))


def check_strips(b, pairs, cm, o, verify):
    want = o["nw"]
    assert b.run().tolist() == [c for c, _ in want], (repr(cm), "run")
    check_traced(pairs, cm, want, b.align(), verify, "align")
    check_traced(pairs, cm, want, b.align_tiled(64), verify, "align_tiled(64)")


def check_dt(b, pairs, cm, o, verify):
    want = o["dt"]
    for s_max in bounds_of(want):
        exp = bounded(want, s_max)
        found = sum(c >= 0 for c, _ in exp)
        assert b.run_dt(s_max).tolist() == [c for c, _ in exp], (repr(cm), "run_dt", s_max)
        info = b.dt_info()
        assert (info["found"], info["not_found"]) == (found, len(pairs) - found), (repr(cm), "run_dt", s_max, info)
        got = b.align_dt(s_max)
        info = b.dt_info()
        assert (info["found"], info["not_found"]) == (found, len(pairs) - found), (repr(cm), "align_dt", s_max, info)
        for p, ((x, y), e, g) in enumerate(zip(pairs, exp, got)):
            assert g == e, (repr(cm), "align_dt", s_max, p, len(x), len(y))
            if g[0] >= 0:
                assert verify(g[1], x, y, cm) == g[0] and ap.no_adjacent_same_op(g[1]), (repr(cm), "align_dt", s_max, p)


def check_dt_seg(b, pairs, cm, o):
    top = bounds_of(o["dt"])[0]
    whole = [(c, g, 0, len(x)) for (x, _), (c, g) in zip(pairs, b.align_dt(top))]
    assert [w[:2] for w in whole] == o["dt"], repr(cm)
    for seg in (0, max_edge(cm), max_edge(cm) + 7):
        got = b.align_dt_seg(top, seg)
        for p, (g, w) in enumerate(zip(got, whole)):
            assert g == w, (repr(cm), "align_dt_seg", seg, p, len(pairs[p][0]), len(pairs[p][1]))
        check_info(b, pairs, got, cm, top, seg, False, False)


def check_ends_free(b, pairs, cm, o, verify):
    """run(), ends(), align() and align_tiled(64) under set_free_ends in all four settings against the ends-free DP; then global again."""
    for fs, fe in SETTINGS:
        want = o["ends"][fs, fe]
        b.set_free_ends(fs, fe)
        assert b.run().tolist() == [w[0] for w in want], (repr(cm), "run", fs, fe)
        assert b.ends().tolist() == [[-1 if fs else 0, w[3]] for w in want], (repr(cm), "ends", fs, fe)
        for what in ("align", "align_tiled"):
            got = b.align() if what == "align" else b.align_tiled(64)
            ends = b.ends().tolist()
            for p, ((x, y), w, (c, g)) in enumerate(zip(pairs, want, got)):
                assert (c, g, ends[p][0], ends[p][1]) == w, (repr(cm), what, fs, fe, p, len(x), len(y))
                assert verify(g, x[w[2]:w[3]], y, cm) == c, (repr(cm), what, fs, fe, p)
    b.set_free_ends(False, False)
    assert b.run().tolist() == [w[0] for w in o["ends"][False, False]], (repr(cm), "run after the ends-free settings")


def check_dt_ends_at(b, pairs, cm, want, s_max, fs, fe, verify):
    exp = bounded4(want, s_max)
    found = sum(w[0] >= 0 for w in exp)
    costs, ends = b.run_dt_ends(s_max, fs, fe)
    assert costs.tolist() == [w[0] for w in exp] and ends.tolist() == [w[3] for w in exp], (repr(cm), "run_dt_ends", s_max, fs, fe)
    info = b.dt_info()
    assert (info["found"], info["not_found"]) == (found, len(pairs) - found), (repr(cm), "run_dt_ends", s_max, fs, fe, info)
    got = b.align_dt_ends(s_max, fs, fe)
    for p, ((x, y), e, g) in enumerate(zip(pairs, exp, got)):
        assert g == e, (repr(cm), "align_dt_ends", s_max, fs, fe, p, len(x), len(y))
        if g[0] >= 0:
            assert verify(g[1], x[g[2]:g[3]], y, cm) == g[0] and ap.no_adjacent_same_op(g[1]), (repr(cm), "align_dt_ends", s_max, fs, fe, p)


def check_dt_ends(b, pairs, cm, o, verify):
    for fs, fe in SETTINGS:
        want = o["dt_ends"][fs, fe]
        check_dt_ends_at(b, pairs, cm, want, max(w[0] for w in want), fs, fe, verify)
    want = o["dt_ends"][True, True]
    check_dt_ends_at(b, pairs, cm, want, max(w[0] for w in want) - 1, True, True, verify)


def check_chained(kind, cm, o, verify):
    pairs, want = cases.long_pairs_for(cm), o["long"]
    b = batch_of(kind)(pairs, cm, trace=True, chain=True)
    try:
        costs = b.run().tolist()
        assert costs == [c for c, _ in want], (repr(cm), "chained run")
        assert b.chain_info()["chain_pairs"] == 2, (repr(cm), b.chain_info())
        tiled = b.align_tiled(64)
        check_traced(pairs, cm, want, tiled, verify, "chained align_tiled(64)")
        b.set_chain(False)
        assert b.run().tolist() == costs and b.align_tiled(64) == tiled, (repr(cm), "the chain off")
    finally:
        b.close()


@pytest.mark.parametrize("kind, name", ALL, ids=["%d-%s" % k for k in ALL])
def test_every_route_under_a_drawn_model(kind, name, oracle):
    cm, o, verify = cases.models(kind)[name], oracle[kind, name], verify_of(kind)
    pairs = cases.pairs_for(cm)
    b = batch_of(kind)(pairs, cm, trace=True)
    try:
        check_strips(b, pairs, cm, o, verify)
        check_dt(b, pairs, cm, o, verify)
        if kind == 2:
            check_dt_seg(b, pairs, cm, o)
        assert b.run().tolist() == [c for c, _ in o["nw"]], (repr(cm), "run after the DT calls")
    finally:
        b.close()
    epairs = cases.ends_pairs_for(cm)
    b = batch_of(kind)(epairs, cm, trace=True)
    try:
        check_ends_free(b, epairs, cm, o, verify)
        check_dt_ends(b, epairs, cm, o, verify)
    finally:
        b.close()
    check_chained(kind, cm, o, verify)


@pytest.mark.parametrize("kind, name", ONE_PER_CLASS, ids=["%d-%s" % k for k in ONE_PER_CLASS])
def test_map_affine_and_map_affine_dt(kind, name, oracle):
    cm, o = cases.models(kind)[name], oracle[kind, name]
    epairs = cases.ends_pairs_for(cm)
    assert pa.map_affine(epairs, cm) == o["ends"][True, True], repr(cm)
    assert pa.map_affine(epairs, cm, free_start=False, tiled=True) == o["ends"][False, True], repr(cm)
    want = o["dt_ends"][True, True]
    top = max(w[0] for w in want)
    assert pa.map_affine_dt(epairs, cm, top) == want, repr(cm)
    assert pa.map_affine_dt(epairs, cm, top - 1) == bounded4(want, top - 1) and NOT_FOUND in bounded4(want, top - 1), repr(cm)
    half = o["dt_ends"][True, False]
    assert pa.map_affine_dt(epairs, cm, max(w[0] for w in half), True, False) == half, repr(cm)


def gpu_costs(pairs, cm):
    b = Affine4Batch(pairs, cm)
    try:
        return b.run().tolist(), b.run_dt(cases.BIG).tolist()
    finally:
        b.close()


def test_layers_are_not_interchangeable():
    """One free model with eight distinct layer numbers against itself with the extends of layers 0 and 2, of 1 and 3, and of both
    pairs exchanged: some pair's cost differs each time, by the oracle and on the GPU, so the sweep above can tell the layers apart (a
    kernel that read extend[1] for extend[3] computes the exchanged model).  Whole layers of one direction exchanged are the same cost
    function, a gap costing the cheaper piece whatever their order: there every cost stays, by the oracle and on the GPU."""
    cm = cases.free_model()
    assert len({x for _, o, e in cm.layers for x in (o, e)}) == 8
    pairs = cases.pairs_for(cm)
    base = [a4.affine4_nw(x, y, cm, trace=False)[0] for x, y in pairs]
    assert gpu_costs(pairs, cm) == (base, base), repr(cm)
    for swap in cases.SWAPS:
        other = cases.swapped(cm, "extend", swap)
        want = [a4.affine4_nw(x, y, other, trace=False)[0] for x, y in pairs]
        assert want != base, (repr(cm), swap)
        assert gpu_costs(pairs, other) == (want, want), (repr(other), swap)
        assert gpu_costs(pairs, cases.swapped(cm, "layer", swap)) == (base, base), (repr(cm), swap)
