"""Both gap-affine batch types at the top of what they accept: every cost component up to 1000 and totals within 0.2 % of 2^30, over the
models and pairs of tests/affine_heavy_cases.py (tests/test_affine_heavy_cases.py says, without a GPU, why they are worth running).  The
diagonal-transition routes (global, ends-free, segmented) against the plain DT oracles with rings of 1001 slots, fronts that are empty
999 times in 1000 and segments of 1000 checkpoint rows; the strip kernels (run, align, align_tiled, chained, ends-free; two and four
layers) against the plain DPs at their shape edges with runs open across the strip row and the tile column; and thin pairs of a
million rows whose costs lie next to kInf against their closed forms.  Every comparison is exact: integers and CIGAR strings.

The DT routes never get s_max = 2^30 - 1 here: under these models the clamp gap_cost(|a|) + gap_cost(|b|) alone would ask for gigabytes
of traced fronts.  The bounds come from the oracle's costs (bounds_of of tests/test_gpu_affine_dt.py).

Measured on an MI355X, the file on its own before the test_dt4_* tests below were added: 76 tests in 81 s, nearly all of it in the
plain oracles (a session that has run tests/test_affine_heavy_cases.py before finds the plain DT's results in
tests/affine_heavy_cases.DT_ORACLE and skips most of that).
Per test: test_dt_global[dt_far-*] 1.9 to 4.8 s (72 000 cost steps a pair under four of the models), test_dt_global[dt_ladder-*] 1.5
to 2.9 s, every other test_dt_global below 1.5 s; test_dt_ends_free 0.1 to 2.3 s; the near-the-limit tests 1.7 to 2.4 s each (the wide
pair's million-step walk by one thread is part of 1.9 to 2.4 s, so it stays traced); test_nw_four_layers 1.1 s; test_nw_two_layers and
its ends-free form 0.6 s; test_dt_every_pair_is_lost_at_its_cost_minus_one 0.7 s; test_dt_segmented at most 0.6 s.

The four-layer DT route (test_dt4_*, 44 tests under the five models of MODELS4; the plain four-layer DT's results come from
affine_heavy_cases.fill_dt4_oracle, in worker processes unless the session has them).  Measured on an MI355X in a session that had run
the CPU module before: test_dt4_global[dt_far-*] 0.5 to 1.0 s (52 600 cost steps under main_edge4), test_dt4_global[dt_ladder-*] at
most 0.5 s, test_dt4_every_pair_is_lost_at_its_cost_minus_one 0.55 s, every other test_dt4_* below 0.5 s; with tests/
test_affine_heavy_cases.py, tests/test_affine_random_cases.py and tests/test_gpu_affine_random.py before it, 290 tests in 90 s."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, capi
from tests import affine4_plain as a4
from tests import affine_heavy_cases as cases
from tests import affine_plain as ap
from tests.affine_dt_ends_plain import affine_dt_ends
from tests.affine_dt_seg_plain import max_edge
from tests.affine_ends_plain import affine_ends
from tests.test_gpu_affine4 import model_pairs
from tests.test_gpu_affine_dt import bounded, bounds_of
from tests.test_gpu_affine_dt_seg import NOT_FOUND, check_info

pytestmark = pytest.mark.gpu

R, R4 = capi.AFFINE_ROWS_PER_LANE, capi.AFFINE4_ROWS_PER_LANE
MODELS, MODELS4 = cases.MODELS, cases.MODELS4
DT = cases.dt_cases()
BIG = (1 << 30) - 1
E = 1000
_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def cached(fn, *key):
    """fn(*key), computed once: the models go in by name."""
    if (fn, key) not in _ORACLE:
        _ORACLE[fn, key] = fn(*key)
    return _ORACLE[fn, key]


def dt_oracle(name, *case_names):
    """(cost, CIGAR) of every pair of the cases by the plain DT (the oracle clamps the bound to the pair's own)."""
    return [r for c in case_names for r in cases.dt_oracle_case(name, c)]


def nw_one(x, y, name):
    return ap.affine_nw(x, y, MODELS[name])


def nw4_one(x, y, name):
    return a4.affine4_nw(x, y, MODELS4[name])


def ends_one(x, y, name, fs, fe):
    return affine_ends(x, y, MODELS[name], fs, fe)[:4]


# ---- diagonal transition, global

def check_dt_at(b, pairs, cm, want, s_max):
    exp = bounded(want, s_max)
    costs = b.run_dt(s_max)
    assert costs.dtype == np.int32 and costs.tolist() == [c for c, _ in exp], s_max
    info = b.dt_info()
    assert info["found"] == sum(c >= 0 for c, _ in exp) and info["found"] + info["not_found"] == len(pairs)
    got = b.align_dt(s_max)
    assert len(got) == len(pairs)
    for p, ((x, y), e, g) in enumerate(zip(pairs, exp, got)):
        assert g == e, (p, len(x), len(y), s_max)
        if g[0] >= 0:
            assert ap.affine_verify(g[1], x, y, cm) == g[0] and ap.no_adjacent_same_op(g[1])
    info = b.dt_info()
    assert info["found"] == sum(c >= 0 for c, _ in exp) and info["found"] + info["not_found"] == len(pairs)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("case", sorted(DT))
def test_dt_global(case, name):
    pairs, cm = DT[case], MODELS[name]
    want = dt_oracle(name, case)
    b = AffineBatch(pairs, cm, trace=True)
    try:
        nw = b.run().tolist()
        assert nw == [c for c, _ in want]  # run() of the same batch gives the same costs
        for s_max in bounds_of(want):  # the largest cost, that minus one (found / not found at cost - 1), the median, 0
            check_dt_at(b, pairs, cm, want, s_max)
        top = bounds_of(want)[0]
        first = (b.run_dt(top).tolist(), b.align_dt(top))
        assert first[1] == want and (b.run_dt(top).tolist(), b.align_dt(top)) == first  # a repeated call gives the same answer
        assert b.run().tolist() == nw
    finally:
        b.close()


def test_dt_every_pair_is_lost_at_its_cost_minus_one():
    """Pair by pair (a batch's bound loses only its most expensive pairs): s_max = cost - 1 is not found, s_max = cost is."""
    for name in ("flat_1000", "coprime", "cheap_sub"):
        pairs = [p for c in ("dt_small", "dt_gap", "dt_runs") for p in DT[c]]
        want = dt_oracle(name, "dt_small", "dt_gap", "dt_runs")
        for (x, y), (c, g) in zip(pairs, want):
            if c == 0:
                continue
            b = AffineBatch([(x, y)], MODELS[name], trace=True)
            try:
                assert b.run_dt(c - 1).tolist() == [-1] and b.align_dt(c - 1) == [(-1, "")]
                assert b.run_dt(c).tolist() == [c] and b.align_dt(c) == [(c, g)]
            finally:
                b.close()


# ---- diagonal transition, ends-free

def dt_ends_one(x, y, name, fs, fe):
    c, st, en, g = affine_dt_ends(x, y, MODELS[name], BIG, fs, fe)
    return c, g, st, en


SETTINGS = ((False, False), (True, False), (False, True), (True, True))  # (free_start, free_end)


@pytest.mark.parametrize("setting", SETTINGS, ids=["fs%d-fe%d" % s for s in SETTINGS])
@pytest.mark.parametrize("name", ("flat_1000", "cheap_sub", "crossover"))
def test_dt_ends_free(name, setting):
    fs, fe = setting
    pairs, cm = cases.dt_planted(), MODELS[name]

    want = [cached(dt_ends_one, x, y, name, fs, fe) for x, y in pairs]
    b = AffineBatch(pairs, cm, trace=True)
    try:
        for s_max in bounds_of([(w[0], w[1]) for w in want]):
            exp = [w if w[0] <= s_max else NOT_FOUND for w in want]
            costs, ends = b.run_dt_ends(s_max, fs, fe)
            assert costs.tolist() == [w[0] for w in exp] and ends.tolist() == [w[3] for w in exp], s_max
            assert b.dt_info()["found"] + b.dt_info()["not_found"] == len(pairs)
            got = b.align_dt_ends(s_max, fs, fe)
            for p, (g, w) in enumerate(zip(got, exp)):
                assert g == w, (p, len(pairs[p][0]), len(pairs[p][1]), s_max)
                if g[0] >= 0:
                    assert ap.affine_verify(g[1], pairs[p][0][g[2]:g[3]], pairs[p][1], cm) == g[0]
    finally:
        b.close()


# ---- diagonal transition, segmented

SEG_ODD = E + 337  # E does not divide it, and it divides no cost of flat_1000


@pytest.mark.parametrize("name", ("flat_1000", "coprime", "cheap_sub", "linear_heavy"))
def test_dt_segmented(name):
    cm = MODELS[name]
    assert max_edge(cm) == E
    pairs = [p for c in cases.SEG_CASES for p in DT[c]]
    want = dt_oracle(name, *cases.SEG_CASES)
    top = max(c for c, _ in want)
    b = AffineBatch(pairs, cm, trace=True)
    try:
        for s_max in sorted({top, top - 1, 0}, reverse=True):
            whole = b.align_dt(s_max)
            assert whole == bounded(want, s_max)
            exp = [(c, g, 0, len(x)) if c >= 0 else NOT_FOUND for (x, _), (c, g) in zip(pairs, whole)]
            for seg in (E, 0, SEG_ODD):
                got = b.align_dt_seg(s_max, seg)
                check_info(b, pairs, got, cm, s_max, seg, False, False)  # the segment counters and the byte formula
                for p, (g, e) in enumerate(zip(got, exp)):
                    assert g == e, (p, len(pairs[p][0]), len(pairs[p][1]), s_max, seg)
        assert b.align_dt_seg(top, E) == b.align_dt_seg(top, E)
        if name != "cheap_sub":
            assert b.dt_seg_info()["rounds"] == top // E + 1 >= 10
    finally:
        b.close()


# ---- the strip kernels, two layers

def check_nw(pairs, cm, want, got, verify):
    assert len(got) == len(pairs)
    for p, ((x, y), w, g) in enumerate(zip(pairs, want, got)):
        assert g == w, (p, len(x), len(y))
        assert verify(g[1], x, y, cm) == g[0] and ap.no_adjacent_same_op(g[1])


@pytest.mark.parametrize("name", sorted(MODELS))
def test_nw_two_layers(name):
    cm = MODELS[name]
    pairs = cases.nw_edges(R)
    want = [cached(nw_one, x, y, name) for x, y in pairs]
    b = AffineBatch(pairs, cm, trace=True)
    try:
        assert b.run().tolist() == [c for c, _ in want]
        check_nw(pairs, cm, want, b.align(), ap.affine_verify)
        check_nw(pairs, cm, want, b.align_tiled(64), ap.affine_verify)
        assert b.run().tolist() == [c for c, _ in want]
    finally:
        b.close()
    long_ = [k for k, (_, y) in enumerate(pairs) if len(y) > 64 * R]
    assert len(long_) >= 6
    sub, subwant = [pairs[k] for k in long_], [want[k] for k in long_]
    b = AffineBatch(sub, cm, trace=True, chain=True)
    try:
        assert b.run().tolist() == [c for c, _ in subwant]
        assert b.chain_info()["chain_pairs"] == len(sub)
        check_nw(sub, cm, subwant, b.align_tiled(64), ap.affine_verify)
    finally:
        b.close()


@pytest.mark.parametrize("name", ("flat_1000", "crossover"))
def test_nw_two_layers_ends_free(name):
    cm = MODELS[name]
    pairs = cases.nw_edges(R)
    want = [cached(ends_one, x, y, name, True, True) for x, y in pairs]
    b = AffineBatch(pairs, cm, trace=True, free_start=True, free_end=True)
    try:
        assert b.run().tolist() == [w[0] for w in want]
        assert b.ends().tolist() == [[-1, w[2]] for w in want]
        for got in (b.align(), b.align_tiled(64)):
            ends = b.ends().tolist()
            for p, ((x, y), w, (c, g)) in enumerate(zip(pairs, want, got)):
                assert (c, ends[p][0], ends[p][1], g) == w, (p, len(x), len(y))
                assert ap.affine_verify(g, x[w[1]:w[2]], y, cm) == c
    finally:
        b.close()


# ---- the strip kernels, four layers

@pytest.mark.parametrize("name", sorted(MODELS4))
def test_nw_four_layers(name):
    cm = MODELS4[name]
    pairs = cases.nw_edges(R4) + model_pairs() + cases.dt_runs()
    want = [cached(nw4_one, x, y, name) for x, y in pairs]
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        assert b.run().tolist() == [c for c, _ in want]
        check_nw(pairs, cm, want, b.align(), a4.affine4_verify)
        check_nw(pairs, cm, want, b.align_tiled(64), a4.affine4_verify)
    finally:
        b.close()


# ---- totals next to 2^30

THIN = [(cm, AffineBatch) for cm in cases.THIN_MODELS.values()] + [(cm, Affine4Batch) for cm in cases.THIN_MODELS4.values()]
thin_params = pytest.mark.parametrize("cm, Batch", THIN, ids=list(cases.THIN_MODELS) + list(cases.THIN_MODELS4))


def ordinary_want(cm, four):
    return [(a4.affine4_nw if four else ap.affine_nw)(x, y, cm) for x, y in cases.ordinary()]


@thin_params
def test_near_the_limit_costs(cm, Batch):
    """All four thin pairs and three ordinary ones in one batch: run(), and run() chained on the two-layer type."""
    four = Batch is Affine4Batch
    thin, exp = cases.thin_limit(cm), cases.thin_expected(cm)
    assert all(cases.LIMIT - cases.LIMIT // 500 <= c < cases.LIMIT for c, _ in exp)
    small, small_want = cases.ordinary(), ordinary_want(cm, four)
    pairs = [thin[0], small[0], thin[1], small[1], thin[2], thin[3], small[2]]
    want = [exp[0][0], small_want[0][0], exp[1][0], small_want[1][0], exp[2][0], exp[3][0], small_want[2][0]]
    b = Batch(pairs, cm)
    try:
        assert b.run().tolist() == want
        if not four:
            b.set_chain(True)
            assert b.run().tolist() == want
            assert b.chain_info()["chain_pairs"] == 2  # the two pairs of a million rows
            b.set_chain(False)
        assert b.run().tolist() == want
    finally:
        b.close()


@thin_params
def test_near_the_limit_tall_pairs_traced(cm, Batch):
    """The two pairs with |a| <= 1 (a million rows, two columns, a thousand strips whose boundary rows hold values next to kInf)
    with three ordinary ones: align() and align_tiled() against the closed forms."""
    four = Batch is Affine4Batch
    thin, exp = cases.thin_limit(cm), cases.thin_expected(cm)
    small, small_want = cases.ordinary(), ordinary_want(cm, four)
    pairs = [small[0], thin[1], small[1], thin[3], small[2]]
    want = [small_want[0], exp[1], small_want[1], exp[3], small_want[2]]
    assert all(len(x) <= 1 for x, _ in (pairs[1], pairs[3]))
    b = Batch(pairs, cm, trace=True)
    try:
        assert b.align() == want
        assert b.align_tiled() == want
        assert b.align_tiled(64) == want
        assert b.run().tolist() == [c for c, _ in want]
    finally:
        b.close()


@thin_params
def test_near_the_limit_wide_pair_traced(cm, Batch):
    """One pair with |b| <= 1 (a million columns; the walk is one thread's million steps): align() against the closed form."""
    four = Batch is Affine4Batch
    thin, exp = cases.thin_limit(cm), cases.thin_expected(cm)
    small, small_want = cases.ordinary(), ordinary_want(cm, four)
    pairs, want = [small[0], thin[2]] + small[1:], [small_want[0], exp[2]] + small_want[1:]
    assert len(pairs[1][1]) == 1
    b = Batch(pairs, cm, trace=True)
    try:
        assert b.align() == want
    finally:
        b.close()


@thin_params
def test_one_byte_more_is_refused(cm, Batch):
    N = cases.thin_n(cm)
    for pair in ((b"A" * (N + 1), b""), (b"", b"A" * (N + 1)), (b"A" * N, b"C")):
        with pytest.raises(ValueError, match=r"pair 1: \(\|a\| \+ \|b\| \+ 1\) \* max edge cost.* is not below 2\^30"):
            Batch([(b"ACGT", b"ACG"), pair], cm)
    # the library's own check, behind the wrapper's
    L = capi.load()
    C = pa.capi.C
    big = b"A" * (N + 1)
    ap_, bp_ = (C.c_char_p * 1)(big), (C.c_char_p * 1)(b"")
    al, bl = np.array([N + 1], np.uint64), np.array([0], np.uint64)
    c = cm.to_c4() if Batch is Affine4Batch else cm.to_c()
    create = L.pa_affine4_batch_create if Batch is Affine4Batch else L.pa_affine_batch_create
    assert not create(ap_, capi._p(al), bp_, capi._p(bl), 1, C.byref(c), 0)
    assert "is not below 2^30" in capi.last_error() and "pair 0" in capi.last_error()


# ---- the four-layer diagonal-transition route

DT4 = cases.dt4_cases()


@pytest.fixture(scope="module")
def dt4_oracle():
    """The plain four-layer DT's word on every list below, in worker processes unless the session has it already."""
    return cases.fill_dt4_oracle(16)


@pytest.mark.parametrize("name", sorted(MODELS4))
@pytest.mark.parametrize("case", sorted(DT4))
def test_dt4_global(case, name, dt4_oracle):
    """check_global of tests/test_gpu_affine4_dt.py under the heavy models: run() gives the oracle's costs, run_dt / align_dt its costs
    and CIGARs at the four bounds of bounds_of, a repeated call the same answer, and run() afterwards is unchanged."""
    from tests.test_gpu_affine4_dt import check_global

    check_global(DT4[case], name, MODELS4[name], cases.dt4_oracle_case(name, case))


def test_dt4_every_pair_is_lost_at_its_cost_minus_one(dt4_oracle):
    """Pair by pair under three models: s_max = cost - 1 is not found, s_max = cost is."""
    for name in cases.DT4_ENDS_MODELS:
        pairs = [p for c in ("dt_small", "dt_gap", "dt_runs") for p in DT4[c]]
        want = [r for c in ("dt_small", "dt_gap", "dt_runs") for r in cases.dt4_oracle_case(name, c)]
        for (x, y), (c, g) in zip(pairs, want):
            if c == 0:
                continue
            b = Affine4Batch([(x, y)], MODELS4[name], trace=True)
            try:
                assert b.run_dt(c - 1).tolist() == [-1] and b.align_dt(c - 1) == [(-1, "")], (name, len(x), len(y), c)
                assert b.run_dt(c).tolist() == [c] and b.align_dt(c) == [(c, g)], (name, len(x), len(y), c)
            finally:
                b.close()


@pytest.mark.parametrize("setting", SETTINGS, ids=["fs%d-fe%d" % s for s in SETTINGS])
@pytest.mark.parametrize("name", cases.DT4_ENDS_MODELS)
def test_dt4_ends_free(name, setting, dt4_oracle):
    """check_ends of tests/test_gpu_affine4_dt.py over dt_planted(): (cost, CIGAR, start, end) of the plain ends-free DT at the bounds
    of bounds_of, and run() / ends() of the same batch under set_free_ends agree on cost and end."""
    from tests.test_gpu_affine4_dt import check_ends

    fs, fe = setting
    check_ends(cases.dt_planted(), name, fs, fe, MODELS4[name], cases.dt4_ends_oracle(name, fs, fe))


def test_dt4_wide_block_at_heavy_costs(dt4_oracle):
    """Four pairs of 300 bytes at 10 % under the dense model: the mean W at the batch's largest cost is above 256, so the block is
    four wavefronts wide, and it meets a main ring of 1001 slots next to layer rings of 2, 2, 3 and 4 (cost only), and traced fronts."""
    from tests.affine4_dt_plain import mean_w
    from tests.test_gpu_affine4_dt import check_global

    cm, pairs, want = MODELS4["dense4"], cases.dt4_wide(), cases.dt4_wide_oracle()
    top = max(c for c, _ in want)
    assert mean_w(pairs, cm, top) > 256
    b = Affine4Batch(pairs, cm)  # cost only: the rings
    try:
        assert b.run_dt(top).tolist() == [c for c, _ in want]
        assert b.run_dt(top - 1).tolist() == [c if c < top else -1 for c, _ in want]
        assert b.run_dt(BIG).tolist() == [c for c, _ in want]
    finally:
        b.close()
    check_global(pairs, "dense4", cm, want)
