"""The segmented traceback of the diagonal-transition route (AffineBatch.align_dt_seg) against AffineBatch.align_dt_ends on the same
batch: equal lists of (cost, CIGAR, start, end), over the pairs of tests/affine_dt_ends_cases.py, four lists of tests/affine_dt_cases.py and
tests/affine_dt_seg_cases.py, with both ends free and globally under all seven models and in every setting under SETTING_MODELS, at
seg = E, E + 1 and the default, and at four bounds (none, the batch's largest cost, that minus one, 0); at the largest cost also
against the plain oracle.  Then the counters, the memory (the header's byte formula, computed here), what the call leaves alone, the
argument errors and the edge batches."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch
from tests import affine_dt_cases as dt_cases
from tests import affine_dt_ends_cases as ends_cases
from tests import affine_dt_seg_cases as cases
from tests import affine_plain as ap
from tests.affine_dt_ends_plain import affine_dt_ends
from tests.affine_dt_plain import reach
from tests.affine_dt_seg_plain import bound_of, max_edge, seg_of

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
MODELS = cases.MODELS
CASES = dict(ends_cases.all_cases(), wide=dt_cases.wide(), far_diagonals=dt_cases.far_diagonals(), low_complexity=dt_cases.low_complexity(),
             mixed=dt_cases.mixed(), **cases.all_cases())
BIG = (1 << 30) - 1
NOT_FOUND = (-1, "", -1, -1)
PARAMS = ([(name, (True, True)) for name in sorted(MODELS)] + [(name, (False, False)) for name in sorted(MODELS)] +
          [(name, s) for name in ends_cases.SETTING_MODELS for s in ((True, False), (False, True))])
_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def oracle(pairs, name, fs, fe):
    """(cost, cigar, start, end) of every pair without a bound by the plain walk; computed once per (pair, model, setting)."""
    out = []
    for x, y in pairs:
        key = (x, y, name, fs, fe)
        if key not in _ORACLE:
            c, st, en, g = affine_dt_ends(x, y, MODELS[name], BIG, fs, fe)
            _ORACLE[key] = (c, g, st, en)
        out.append(_ORACLE[key])
    return out


def pair_shape(n, m, cm, s_max, fs, fe):
    """(s', layers, W) of a pair by the host's rule (include/pa_affine_hip.h, pa_affine_batch_run_dt_ends)."""
    sub, ins, dl, io, ie, do, de = ap.edge_costs(cm)
    sb = bound_of(n, m, cm, s_max, fs, fe)
    back = reach(sb, ins, io, ie)
    kmin = -min(m, back)
    kmax = min(n, max(0, n - m + back)) if fs else min(n, reach(sb, dl, do, de))
    return sb, 3 if (io is not None or do is not None) else 1, kmax - kmin + 3


def ends_bytes(n, m, cm, s_max, fs, fe):
    """Device bytes of a pair in align_dt_ends: every front up to s', the kNeg row, the ops."""
    sb, L, W = pair_shape(n, m, cm, s_max, fs, fe)
    return (sb + 2) * L * W * 4 + ((n + m + 15) & ~15)


def seg_bytes(n, m, cm, s_max, seg, fs, fe):
    """Device bytes of a pair in align_dt_seg, by the header's formula."""
    sb, L, W = pair_shape(n, m, cm, s_max, fs, fe)
    E = max_edge(cm)
    S = seg_of(sb, E, seg)
    nseg = sb // S + 1
    return ((E + 2) + (nseg - 1) * E + (E + S + 1)) * L * W * 4 + ((n + m + 15) & ~15) + 40


def nsegs(pairs, got, cm, s_max, seg, fs, fe):
    """cost / S + 1 of every found pair, S the pair's segment length."""
    E = max_edge(cm)
    return [g[0] // seg_of(bound_of(len(x), len(y), cm, s_max, fs, fe), E, seg) + 1 for (x, y), g in zip(pairs, got) if g[0] >= 0]


def check_info(b, pairs, got, cm, s_max, seg, fs, fe):
    """The counters of a call that ran in one chunk follow from the costs and seg alone; bytes_max from the header's formula."""
    info, ck = b.dt_seg_info(), b.dt_info()
    ns = nsegs(pairs, got, cm, s_max, seg, fs, fe)
    assert info["chunks"] == 1 and info["rounds"] == max(ns, default=0) and info["seg_jobs"] == sum(ns)
    assert (info["refill_cells"] > 0) == bool(ns)
    assert info["bytes_max"] == sum(seg_bytes(len(x), len(y), cm, s_max, seg, fs, fe) for x, y in pairs) == ck["bytes_max"]
    assert ck["found"] == len(ns) and ck["found"] + ck["not_found"] == len(pairs) and ck["chunks"] == 1 and ck["front_cells"] > 0


def check_batch(pairs, name, fs, fe):
    cm = MODELS[name]
    E = max_edge(cm)
    want = oracle(pairs, name, fs, fe)
    top = max(w[0] for w in want)
    b = AffineBatch(pairs, cm, trace=True)
    try:
        for s_max in [BIG] + sorted({top, max(top - 1, 0), 0}, reverse=True):
            ends = b.align_dt_ends(s_max, fs, fe)
            if s_max == top:  # the plain oracle, and every CIGAR priced on its own
                assert ends == want
            for seg in (E, E + 1, 0):
                got = b.align_dt_seg(s_max, seg, fs, fe)
                assert len(got) == len(pairs)
                for p, (g, e) in enumerate(zip(got, ends)):
                    assert g == e, (p, len(pairs[p][0]), len(pairs[p][1]), s_max, seg)
                check_info(b, pairs, got, cm, s_max, seg, fs, fe)
                if s_max == top:
                    for (x, y), g in zip(pairs, got):
                        assert ap.affine_verify(g[1], x[g[2]:g[3]], y, cm) == g[0] and ap.no_adjacent_same_op(g[1])
    finally:
        b.close()


@pytest.mark.parametrize("name,setting", PARAMS, ids=["%s-fs%d-fe%d" % (n, *s) for n, s in PARAMS])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_same_batch_the_two_routes(case, name, setting):
    check_batch(CASES[case], name, *setting)


@pytest.mark.parametrize("name", ("affine", "unit", "linear_asymmetric"))
def test_both_switches_off_is_align_dt(name):
    pairs = CASES["gaps"] + CASES["ladder"] + CASES["tails"][::4] + CASES["windows"][:3]
    b = AffineBatch(pairs, MODELS[name], trace=True)
    try:
        for s_max in (BIG, 12, 0):
            want = b.align_dt(s_max)
            for seg in (0, max_edge(MODELS[name])):
                got = b.align_dt_seg(s_max, seg)
                assert got == [(c, g, 0, len(x)) if c >= 0 else NOT_FOUND for (x, _), (c, g) in zip(pairs, want)]
    finally:
        b.close()


def test_counters():
    pairs = CASES["gaps"] + CASES["small"] + CASES["ladder"] + CASES["wide"]
    cm = MODELS["affine"]
    b = AffineBatch(pairs, cm, trace=True)
    try:
        want = b.align_dt_ends(BIG, False, False)
        top = max(w[0] for w in want)
        for s_max, seg in ((BIG, 8), (BIG, 0), (top, 0), (86, 6), (top - 1, 7)):
            got = b.align_dt_seg(s_max, seg)
            assert got == [w if w[0] <= s_max else NOT_FOUND for w in want]
            check_info(b, pairs, got, cm, s_max, seg, False, False)
        assert b.align_dt_seg(BIG, 8)[0][0] == 86 and b.dt_seg_info()["rounds"] == top // 8 + 1 > 11
        assert b.align_dt_seg(BIG, top + 1) == want  # a seg above every cost: one round
        info = b.dt_seg_info()
        assert info["rounds"] == info["chunks"] == 1 and info["seg_jobs"] == len(pairs) and info["refill_cells"] > 0
        assert b.last_forward_ms > 0 and b.last_refill_ms > 0 and b.last_trace_ms > 0
    finally:
        b.close()


_CHILD = """
import json, sys
from astar_pairwise_aligner_amd import AffineBatch
from tests import affine_dt_cases, affine_dt_ends_cases as cases
name, s_max, fs = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
pairs = affine_dt_cases.mixed() if name == "mixed" else cases.windows() * 6
b = AffineBatch(pairs, cases.MODELS["affine"], trace=True)
out = {}
try:
    b.align_dt_ends(s_max, fs, fs)
    out["ends_error"] = None
except ValueError as e:
    out["ends_error"] = str(e)
out["seg"] = b.align_dt_seg(s_max, 0, fs, fs)
out["info"] = b.dt_seg_info()
b.close()
print(json.dumps(out))
"""


def child(name, s_max, fs, budget_mb):
    env = dict(os.environ, PA_AFFINE_TRACE_BUDGET_MB=repr(budget_mb))
    r = subprocess.run([sys.executable, "-c", _CHILD, name, str(s_max), str(int(fs))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_memory_is_below_that_of_every_front():
    pairs = CASES["mixed"]
    cm = MODELS["affine"]
    want = oracle(pairs, "affine", False, False)
    top = max(w[0] for w in want)
    b = AffineBatch(pairs, cm, trace=True)
    try:
        assert b.align_dt_ends(top, False, False) == want
        every = b.dt_info()["bytes_max"]
        assert b.align_dt_seg(top) == want
        assert b.dt_seg_info()["bytes_max"] < every and b.dt_seg_info()["chunks"] == 1
        assert every == sum(ends_bytes(len(x), len(y), cm, top, False, False) for x, y in pairs)
    finally:
        b.close()
    # a budget between the two figures of the 2.9 kbp pair: every front of it does not fit, its segments do
    big = max(range(len(pairs)), key=lambda p: len(pairs[p][0]))
    n, m = len(pairs[big][0]), len(pairs[big][1])
    assert n == 2900
    lo, hi = seg_bytes(n, m, cm, top, 0, False, False), ends_bytes(n, m, cm, top, False, False)
    assert lo < hi / 4
    budget = (lo + hi) / 2
    out = child("mixed", top, False, budget / 1048576)
    assert out["ends_error"] is not None and "exceed the budget" in out["ends_error"]
    named = int(re.search(r"pair (\d+):", out["ends_error"]).group(1))  # the first pair that does not fit: that one, or the 2.1 kbp pair
    assert named <= big and ends_bytes(len(pairs[named][0]), len(pairs[named][1]), cm, top, False, False) > budget
    assert all(seg_bytes(len(x), len(y), cm, top, 0, False, False) <= budget for x, y in pairs)
    assert [tuple(x) for x in out["seg"]] == want
    assert out["info"]["bytes_max"] <= budget


def test_small_budget_chunks_with_the_same_results():
    pairs = ends_cases.windows() * 6
    cm = MODELS["affine"]
    want = oracle(pairs, "affine", True, True)
    s_max = max(w[0] for w in want) - 1
    exp = [w if w[0] <= s_max else NOT_FOUND for w in want]
    per_pair = [seg_bytes(len(x), len(y), cm, s_max, 0, True, True) for x, y in pairs]
    budget = max(2 * max(per_pair), sum(per_pair) // 5)  # several chunks, and room for every pair
    assert budget < sum(per_pair) / 2
    out = child("windows", s_max, True, budget / 1048576)
    assert out["ends_error"] is None
    assert [tuple(x) for x in out["seg"]] == exp
    assert out["info"]["chunks"] > 1 and out["info"]["bytes_max"] <= budget
    b = AffineBatch(pairs, cm, trace=True)  # the default budget: one chunk
    try:
        assert b.align_dt_seg(s_max, 0, True, True) == exp
        info = b.dt_seg_info()
        assert info["chunks"] == 1 and info["seg_jobs"] == out["info"]["seg_jobs"] and info["refill_cells"] == out["info"]["refill_cells"]
        assert out["info"]["rounds"] >= info["rounds"]
    finally:
        b.close()


def test_the_call_leaves_the_batch_alone():
    pairs = ends_cases.flanked()[::3] + CASES["tied"] + CASES["gaps"]
    cm = MODELS["affine"]
    b = AffineBatch(pairs, cm, trace=True)
    try:
        nw, dt = b.run().tolist(), b.run_dt(BIG).tolist()
        glob_ends = b.ends().tolist()
        first = b.align_dt_seg(BIG, 0, True, False)
        assert first == b.align_dt_ends(BIG, True, False)
        assert b.align_dt_seg(BIG, 0, True, False) == first  # a repeated call is identical
        b.align_dt_seg(BIG, 8)
        assert b.ends().tolist() == glob_ends
        assert b.run_dt(BIG).tolist() == dt and b.run().tolist() == nw  # the batch is still global: run_dt() does not refuse it
        b.set_free_ends(True, True)
        free, free_ends = b.run().tolist(), b.ends().tolist()
        got = b.align_dt_seg(BIG, 7)  # the call's switches (both off), not the batch's
        assert [g[0] for g in got] == dt and [g[3] for g in got] == [len(x) for x, _ in pairs] and all(g[2] == 0 for g in got)
        assert b.ends().tolist() == free_ends and b.run().tolist() == free
        with pytest.raises(ValueError, match="pa_affine_batch_run_dt: .*ends-free"):  # the setting is still on
            b.run_dt(10)
        b.set_chain(True)  # ignored
        assert [g[0] for g in b.align_dt_seg(BIG, 0, True, True)] == free
        assert b.chain_info()["on"] is True
    finally:
        b.close()


def test_argument_errors():
    pairs = CASES["tails"][:5]
    L = pa.capi.load()
    fn = "pa_affine_batch_align_dt_seg"
    none = (None,) * 7
    b = AffineBatch(pairs, MODELS["affine"])  # no trace
    try:
        with pytest.raises(ValueError, match=fn + ": the batch was created without trace"):
            b.align_dt_seg(10)
        assert L.pa_affine_batch_align_dt_seg(b._h, 0, 0, 5, 0, *none) == -4
    finally:
        b.close()
    b = AffineBatch(pairs, MODELS["affine"], trace=True)  # the largest edge is 6
    try:
        for seg in (1, 5):
            with pytest.raises(ValueError, match=fn + ": seg = %d .*largest edge is 6" % seg):
                b.align_dt_seg(10, seg)
        assert len(b.align_dt_seg(10, 6)) == 5
        assert L.pa_affine_batch_align_dt_seg(b._h, 0, 0, 5, 1 << 30, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "seg" in pa.capi.last_error() and "largest edge" in pa.capi.last_error()
        assert L.pa_affine_batch_align_dt_seg(b._h, 2, 0, 5, 0, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "free_start" in pa.capi.last_error()
        assert L.pa_affine_batch_align_dt_seg(b._h, 0, -1, 5, 0, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "free_end" in pa.capi.last_error()
        assert L.pa_affine_batch_align_dt_seg(b._h, 1, 1, -1, 0, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "s_max" in pa.capi.last_error()
        assert L.pa_affine_batch_align_dt_seg(b._h, 1, 1, 5, 0, *none) == 0  # every output is optional
        assert b.dt_seg_info()["chunks"] == 1
    finally:
        b.close()


def test_edge_batches():
    b = AffineBatch([], MODELS["affine"], trace=True)
    try:
        assert b.align_dt_seg(5) == [] and b.align_dt_seg(5, 9, True, True) == []
        assert b.dt_seg_info() == dict(chunks=0, rounds=0, seg_jobs=0, refill_cells=0, bytes_max=0)
    finally:
        b.close()
    pairs = [p for p in CASES["ladder"]]  # unequal pairs: none is found at s_max = 0
    b = AffineBatch(pairs, MODELS["affine"], trace=True)
    try:
        assert b.align_dt_seg(0) == [NOT_FOUND] * len(pairs)
        info = b.dt_seg_info()
        assert info["chunks"] == 1 and info["rounds"] == 0 and info["seg_jobs"] == 0 and info["refill_cells"] == 0 and info["bytes_max"] > 0
        assert b.dt_info()["found"] == 0 and b.dt_info()["not_found"] == len(pairs)
    finally:
        b.close()
