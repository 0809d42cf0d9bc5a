"""The ends-free diagonal-transition route of the batched gap-affine aligner (AffineBatch.run_dt_ends / align_dt_ends, map_affine(s_max=))
against the plain restatement of tests/affine_dt_ends_plain.py: cost, start, end and exact CIGAR string over the pairs of
tests/affine_dt_ends_cases.py, every setting under SETTING_MODELS and both ends free under all seven models, at four values of s_max (the
batch's largest cost, that minus one, 0, and none); plus the cost and end of the ends-free AffineBatch.run(), and what the calls must leave alone."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch
from tests import affine_dt_ends_cases as cases
from tests import affine_plain as ap
from tests.affine_dt_ends_plain import affine_dt_ends

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
MODELS = cases.MODELS
CASES = cases.all_cases()
BIG = (1 << 30) - 1
NOT_FOUND = (-1, "", -1, -1)
_ORACLE = {}
PARAMS = [(name, s) for name in sorted(MODELS) for s in cases.SETTINGS if name in cases.SETTING_MODELS or s == (True, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def oracle(pairs, name, fs, fe):
    """(cost, cigar, start, end) of every pair without a bound, in align_dt_ends' order; computed once per (pair, model, setting)."""
    out = []
    for x, y in pairs:
        key = (x, y, name, fs, fe)
        if key not in _ORACLE:
            c, st, en, g = affine_dt_ends(x, y, MODELS[name], BIG, fs, fe)
            _ORACLE[key] = (c, g, st, en)
        out.append(_ORACLE[key])
    return out


def bounded(want, s_max):
    return [w if w[0] <= s_max else NOT_FOUND for w in want]


def bounds_of(want):
    """The batch's largest cost (everything found), that minus one (exactly the most expensive pairs are not), and 0; and no bound,
    where the host trims no diagonal and front 0 under free_start is |a| + 1 wide."""
    top = max(w[0] for w in want)
    return [BIG] + sorted({top, max(top - 1, 0), 0}, reverse=True)


def check_at(b, pairs, name, fs, fe, want, s_max):
    exp = bounded(want, s_max)
    costs, ends = b.run_dt_ends(s_max, fs, fe)
    assert costs.dtype == np.int32 and ends.dtype == np.int64
    assert costs.tolist() == [w[0] for w in exp] and ends.tolist() == [w[3] for w in exp], s_max
    info = b.dt_info()
    assert info["found"] == sum(w[0] >= 0 for w in exp) and info["found"] + info["not_found"] == len(pairs)
    assert info["front_cells"] > 0 and info["chunks"] >= 1 and info["bytes_max"] > 0
    got = b.align_dt_ends(s_max, fs, fe)
    assert len(got) == len(pairs)
    for p, ((x, y), e, g) in enumerate(zip(pairs, exp, got)):
        assert g == e, (p, len(x), len(y), s_max)
        if g[0] >= 0:
            assert ap.affine_verify(g[1], x[g[2]:g[3]], y, MODELS[name]) == g[0] and ap.no_adjacent_same_op(g[1])
    assert b.dt_info()["found"] == info["found"] and b.dt_info()["found"] + b.dt_info()["not_found"] == len(pairs)


def check_batch(pairs, name, fs, fe):
    want = oracle(pairs, name, fs, fe)
    b = AffineBatch(pairs, MODELS[name], trace=True)
    try:
        for s_max in bounds_of(want):
            check_at(b, pairs, name, fs, fe, want, s_max)
        top = bounds_of(want)[0]
        first = ([r.tolist() for r in b.run_dt_ends(top, fs, fe)], b.align_dt_ends(top, fs, fe))
        assert ([r.tolist() for r in b.run_dt_ends(top, fs, fe)], b.align_dt_ends(top, fs, fe)) == first  # a repeated call is identical
        # cost and end are those of the ends-free DP of the same batch
        b.set_free_ends(fs, fe)
        assert b.run().tolist() == first[0][0] and b.ends()[:, 1].tolist() == first[0][1]
    finally:
        b.close()


@pytest.mark.parametrize("name,setting", PARAMS, ids=["%s-fs%d-fe%d" % (n, *s) for n, s in PARAMS])
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_case_list_model_and_setting(case, name, setting):
    check_batch(CASES[case], name, *setting)


def test_tied_ends_across_the_wavefronts_of_a_wide_block():
    """tied's first pairs among windows: the batch's mean W is above 256, so the eight tied ends of y * 8 lie in the four wavefronts of
    one block, and the lowest must win."""
    pairs = CASES["tied"][:2] + CASES["windows"]
    for name in ("affine", "unit"):
        check_batch(pairs, name, True, True)
        b = AffineBatch(pairs, MODELS[name])
        try:
            costs, ends = b.run_dt_ends(BIG)
            assert (costs[0], ends[0]) == (0, 40)
        finally:
            b.close()


def test_the_calls_leave_the_batch_alone():
    pairs = CASES["flanked"][::3] + CASES["tied"]
    cm = MODELS["affine"]
    b = AffineBatch(pairs, cm, trace=True)
    try:
        nw, dt = b.run().tolist(), b.run_dt(BIG).tolist()
        glob_ends = b.ends().tolist()
        b.run_dt_ends(BIG)
        b.align_dt_ends(BIG, True, False)
        assert b.ends().tolist() == glob_ends                      # still the global run()'s
        assert b.run_dt(BIG).tolist() == dt and b.run().tolist() == nw  # the batch is still global: run_dt() does not refuse it
        b.set_free_ends(True, True)
        free, free_ends = b.run().tolist(), b.ends().tolist()
        costs, ends = b.run_dt_ends(BIG, False, False)             # the call's switches, not the batch's
        assert costs.tolist() == dt and ends.tolist() == [len(x) for x, _ in pairs]
        assert b.ends().tolist() == free_ends and b.run().tolist() == free
        with pytest.raises(ValueError, match="pa_affine_batch_run_dt: .*ends-free"):  # the setting is still on
            b.run_dt(10)
        b.set_chain(True)  # ignored
        assert b.run_dt_ends(BIG)[0].tolist() == free
    finally:
        b.close()


@pytest.mark.parametrize("name", ("affine", "unit", "linear_asymmetric"))
def test_both_switches_off_is_the_global_route(name):
    pairs = CASES["tails"][::4] + CASES["lengths"][::9] + CASES["windows"][:3]
    b = AffineBatch(pairs, MODELS[name], trace=True)
    try:
        for s_max in (BIG, 12, 0):
            want_c, want = b.run_dt(s_max).tolist(), b.align_dt(s_max)
            info = b.dt_info()
            costs, ends = b.run_dt_ends(s_max, False, False)
            assert costs.tolist() == want_c and ends.tolist() == [len(x) if c >= 0 else -1 for (x, _), c in zip(pairs, want_c)]
            got = b.align_dt_ends(s_max, False, False)
            assert got == [(c, g, 0, len(x)) if c >= 0 else NOT_FOUND for (x, _), (c, g) in zip(pairs, want)]
            assert b.dt_info() == info
    finally:
        b.close()


def test_argument_errors():
    pairs = CASES["tails"][:5]
    b = AffineBatch(pairs, MODELS["affine"])  # no trace
    try:
        with pytest.raises(ValueError, match="pa_affine_batch_align_dt_ends: the batch was created without trace"):
            b.align_dt_ends(10)
        assert len(b.run_dt_ends(10)[0]) == 5
        L = pa.capi.load()
        assert L.pa_affine_batch_run_dt_ends(b._h, 1, 1, -1, None, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine_batch_run_dt_ends:") and "s_max" in pa.capi.last_error()
        assert L.pa_affine_batch_run_dt_ends(b._h, 2, 0, 5, None, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine_batch_run_dt_ends:") and "free_start" in pa.capi.last_error()
        assert L.pa_affine_batch_align_dt_ends(b._h, 0, -1, 5, None, None, None, None, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine_batch_align_dt_ends:") and "free_end" in pa.capi.last_error()
        assert L.pa_affine_batch_run_dt_ends(b._h, 1, 1, 5, None, None, None) == 0  # every output is optional
    finally:
        b.close()


def test_empty_batch():
    b = AffineBatch([], MODELS["affine"], trace=True)
    try:
        costs, ends = b.run_dt_ends(5)
        assert costs.tolist() == [] and ends.tolist() == [] and b.align_dt_ends(5) == []
        assert b.dt_info()["found"] == 0 and b.dt_info()["not_found"] == 0
    finally:
        b.close()
    assert pa.map_affine([], MODELS["affine"], s_max=3) == []


def test_map_affine_with_a_bound_is_align_dt_ends():
    pairs = CASES["packed_unequal"] + CASES["tied"]
    cm = MODELS["affine"]
    want = oracle(pairs, "affine", True, True)
    K = bounds_of(want)[2]  # the largest cost minus one
    assert pa.map_affine(pairs, cm, s_max=K) == bounded(want, K)
    half = oracle(pairs, "affine", False, True)
    assert pa.map_affine(pairs, cm, free_start=False, s_max=BIG) == half
    b = AffineBatch(pairs, cm, trace=True)
    try:
        assert b.align_dt_ends(K) == pa.map_affine(pairs, cm, s_max=K)
    finally:
        b.close()
    # cost and end (not start and CIGAR, which may be another optimal placement) are those of the DP route
    assert [(c, e) for c, _, _, e in pa.map_affine(pairs, cm, s_max=BIG)] == [(c, e) for c, _, _, e in pa.map_affine(pairs, cm)]


_CHILD = """
import json, sys
from astar_pairwise_aligner_amd import AffineBatch
from tests import affine_dt_ends_cases as cases
pairs = cases.windows() * 6
s_max = int(sys.argv[1])
b = AffineBatch(pairs, cases.MODELS["affine"], trace=True)
costs, ends = b.run_dt_ends(s_max)
out = {"run": [costs.tolist(), ends.tolist()], "run_info": b.dt_info()}
out["align"] = b.align_dt_ends(s_max)
out["align_info"] = b.dt_info()
b.close()
print(json.dumps(out))
"""


def test_small_budget_chunks_with_the_same_results():
    """PA_AFFINE_TRACE_BUDGET_MB = 2 in a fresh child process: the rings of windows * 6 (114 pairs, about 40 KB each under free_start) take
    more than one chunk and their traced fronts many, with the results and counters of the default budget."""
    pairs = cases.windows() * 6
    want = oracle(pairs, "affine", True, True)
    s_max = max(w[0] for w in want) - 1
    env = dict(os.environ, PA_AFFINE_TRACE_BUDGET_MB="2")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(s_max)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    exp = bounded(want, s_max)
    assert out["run"] == [[w[0] for w in exp], [w[3] for w in exp]] and [tuple(x) for x in out["align"]] == exp
    assert out["run_info"]["chunks"] > 1 and out["run_info"]["bytes_max"] <= 2 << 20
    assert out["align_info"]["chunks"] > out["run_info"]["chunks"] and out["align_info"]["bytes_max"] <= 2 << 20
    assert out["run_info"]["found"] + out["run_info"]["not_found"] == len(pairs) and out["run_info"]["not_found"] >= 6
    b = AffineBatch(pairs, MODELS["affine"], trace=True)  # the default budget: one chunk
    try:
        costs, ends = b.run_dt_ends(s_max)
        assert [costs.tolist(), ends.tolist()] == out["run"] and b.dt_info()["chunks"] == 1
        assert b.dt_info()["front_cells"] == out["run_info"]["front_cells"] and b.dt_info()["extend_chars"] == out["run_info"]["extend_chars"]
        assert b.align_dt_ends(s_max) == exp
    finally:
        b.close()
