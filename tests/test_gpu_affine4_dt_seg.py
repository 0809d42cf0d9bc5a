"""The segmented traceback of the double-affine diagonal-transition route (Affine4Batch.align_dt_segmented) against
Affine4Batch.align_dt_ends on the same batch: equal lists of (cost, CIGAR, start, end), over the ends-free and the global lists of
tests/affine4_dt_cases.py and the lists of tests/affine4_dt_seg_cases.py, under the three models of the DT tests and STEEP, Ew above E
(every list under all four; the 2 .. 3 kbp lists under double_affine, one of them under STEEP too), with both ends free and
globally, and in the two one-sided settings under double_affine, at seg = Ew, Ew + 1 and the default, and at four
bounds (none, the batch's largest cost, that minus one, 0); at the largest cost also against the plain oracle, every CIGAR priced on its
own.  Then the counters, the memory (the header's byte formula, computed here), what the call leaves alone, the refusals, the edge
batches, a budget in a child process, and the heavy and the seeded random models.

The plain oracle runs once per (pair, model, setting) of this module: 30 s in all on the box's host, most of it on the lists of
150 to 200 short pairs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch
from tests import affine4_dt_cases as dt4_cases
from tests import affine4_dt_seg_cases as cases
from tests import affine_heavy_cases as heavy
from tests import affine_plain as ap
from tests import affine_random_cases as rnd
from tests.affine4_dt_plain import affine4_dt, bound_of, mean_w, reach
from tests.affine4_dt_seg_plain import Ew, H, heads, seg_of
from tests.affine4_plain import _model, affine4_verify

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
MODELS = cases.MODELS
ENDS = dt4_cases.ends_cases_all()
GLOBAL = dt4_cases.global_cases()
NEW = cases.new_cases()
CASES = dict({"ends_" + k: v for k, v in ENDS.items()}, **{"global_" + k: v for k, v in GLOBAL.items()}, **NEW, many=cases.many())
LONG = ("ends_long", "global_mixed", "many")  # 2 .. 3 kbp: double_affine only, and wide blocks
BIG = (1 << 30) - 1
NOT_FOUND = (-1, "", -1, -1)
FREE, GLOB = (True, True), (False, False)
ONE_SIDED = ((True, False), (False, True))
_ORACLE = {}


def _params():
    """Every list under the four models; the 2 .. 3 kbp lists (LONG) under double_affine alone, the numpy oracle taking seconds a pair
    there, and `many` also under STEEP, whose blocks it makes wide (a mean W of 287 at its cost of 1132; every other list is narrow
    under STEEP, whose extends of 8 and 9 reach an eighth as far as an extend of 1).  The ends-free lists run with both ends free and
    the global lists globally, as in tests/test_gpu_affine4_dt.py, and the new lists both ways; under double_affine the ends-free and
    the new lists also run in the other settings."""
    out = []
    for case in sorted(CASES):
        for name in ["double_affine"] if case in LONG else sorted(MODELS):
            both = name == "double_affine"
            if case.startswith("ends_"):
                out += [(case, name, s) for s in ((FREE, GLOB) + ONE_SIDED if both else (FREE,))]
            elif case.startswith("global_"):
                out.append((case, name, GLOB))
            else:
                out += [(case, name, s) for s in (FREE, GLOB) + (ONE_SIDED if both and case != "many" else ())]
    return out + [("many", "steep", GLOB)]


PARAMS = _params()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def oracle(pairs, name, fs, fe):
    """(cost, cigar, start, end) of every pair without a bound by the plain walk; computed once per (pair, model, setting)."""
    out = []
    for x, y in pairs:
        key = (x, y, name, fs, fe)
        if key not in _ORACLE:
            _ORACLE[key] = affine4_dt(x, y, MODELS[name], BIG, fs, fe)
        out.append(_ORACLE[key])
    return out


def pair_shape(n, m, cm, s_max, fs, fe):
    """(s', W) of a pair by the host's rule (csrc/affine4_dt_plan.hpp shape_of, restated)."""
    _, ins, dl, op, ex = _model(cm)
    sb = bound_of(n, m, cm, s_max, fs, fe)
    back = reach(sb, ins, [(op[0], ex[0]), (op[2], ex[2])])
    kmin = -min(m, back)
    kmax = min(n, max(0, n - m + back)) if fs else min(n, reach(sb, dl, [(op[1], ex[1]), (op[3], ex[3])]))
    return sb, kmax - kmin + 3


def ends_bytes(n, m, cm, s_max, fs, fe):
    """Device bytes of a pair in align_dt_ends (include/pa_affine4_dt_hip.h): every front up to s', the kNeg row, the ops."""
    sb, W = pair_shape(n, m, cm, s_max, fs, fe)
    return (5 * (sb + 1) + 1) * W * 4 + ((n + m + 15) & ~15)


def seg_bytes(n, m, cm, s_max, seg, fs, fe):
    """Device bytes of a pair in align_dt_segmented, by the formula of include/pa_affine4_dt_seg_hip.h."""
    sb, W = pair_shape(n, m, cm, s_max, fs, fe)
    S = seg_of(sb, cm, seg)
    nseg = sb // S + 1
    ring = sum(h + 1 for h in heads(cm)) + 1
    return (ring + (nseg - 1) * H(cm) + H(cm) + 5 * S + 1) * W * 4 + ((n + m + 15) & ~15) + 40


def nsegs(pairs, got, cm, s_max, seg, fs, fe):
    """cost / S + 1 of every found pair, S the pair's segment length."""
    return [g[0] // seg_of(bound_of(len(x), len(y), cm, s_max, fs, fe), cm, seg) + 1 for (x, y), g in zip(pairs, got) if g[0] >= 0]


def check_info(b, pairs, got, cm, s_max, seg, fs, fe):
    """The counters of a call that ran in one chunk follow from the costs and seg alone; bytes_max from the header's formula."""
    info, ck = b.dt_segmented_info(), b.dt_info()
    ns = nsegs(pairs, got, cm, s_max, seg, fs, fe)
    assert info["chunks"] == 1 and info["rounds"] == max(ns, default=0) and info["seg_jobs"] == sum(ns)
    assert (info["refill_cells"] > 0) == bool(ns)
    assert info["bytes_max"] == sum(seg_bytes(len(x), len(y), cm, s_max, seg, fs, fe) for x, y in pairs) == ck["bytes_max"]
    assert ck["found"] == len(ns) and ck["found"] + ck["not_found"] == len(pairs) and ck["chunks"] == 1 and ck["front_cells"] > 0


def check_batch(pairs, cm, fs, fe, want=None, bounds=None, segs=None):
    """align_dt_segmented against align_dt_ends of the same batch at every bound (none, the largest cost, that minus one, 0; with
    bounds = "top" the two in the middle, where every front of a loose bound would be gigabytes) and seg; with `want`, the plain
    oracle's results without a bound, also against those at the largest cost, with every CIGAR priced."""
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        top = max(w[0] for w in want) if want else int(b.run_dt_ends(BIG, fs, fe)[0].max())
        at_top = sorted({top, max(top - 1, 0)}, reverse=True)
        for s_max in at_top if bounds == "top" else [BIG] + at_top + [0] * (top > 1):
            ends = b.align_dt_ends(s_max, fs, fe)
            if want and s_max == top:
                assert ends == want
            for seg in segs or (Ew(cm), Ew(cm) + 1, 0):
                got = b.align_dt_segmented(s_max, seg, fs, fe)
                assert len(got) == len(pairs)
                for p, (g, e) in enumerate(zip(got, ends)):
                    assert g == e, (p, len(pairs[p][0]), len(pairs[p][1]), s_max, seg)
                check_info(b, pairs, got, cm, s_max, seg, fs, fe)
                if want and s_max == top:
                    for (x, y), g in zip(pairs, got):
                        assert affine4_verify(g[1], x[g[2]:g[3]], y, cm) == g[0] and ap.no_adjacent_same_op(g[1])
    finally:
        b.close()


@pytest.mark.parametrize("case,name,setting", PARAMS, ids=["%s-%s-fs%d-fe%d" % (c, n, *s) for c, n, s in PARAMS])
def test_the_same_batch_the_two_routes(case, name, setting):
    pairs, cm = CASES[case], MODELS[name]
    want = oracle(pairs, name, *setting)
    wide = mean_w(pairs, cm, max(w[0] for w in want), *setting) > dt4_cases.WIDE_MEAN
    assert wide or case not in LONG  # the 2 .. 3 kbp lists run in wide blocks
    assert not (wide and case in NEW)  # and the short new lists in narrow ones
    check_batch(pairs, cm, *setting, want=want)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_both_switches_off_is_align_dt(name):
    pairs = NEW["long_gap"] + NEW["ladder"] + GLOBAL["tails"][::4] + ENDS["windows"][:3] + cases.gap18()
    cm = MODELS[name]
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        for s_max in (BIG, 42, 0):
            want = b.align_dt(s_max)
            for seg in (0, Ew(cm)):
                got = b.align_dt_segmented(s_max, seg)
                assert got == [(c, g, 0, len(x)) if c >= 0 else NOT_FOUND for (x, _), (c, g) in zip(pairs, want)]
    finally:
        b.close()


def test_counters():
    pairs = NEW["long_gap"] + NEW["small"] + NEW["ladder"] + GLOBAL["wide"] + cases.gap18()
    cm = MODELS["double_affine"]
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        want = b.align_dt_ends(BIG, False, False)
        assert want == oracle(pairs, "double_affine", False, False)
        top = max(w[0] for w in want)
        for s_max, seg in ((BIG, 24), (BIG, 0), (top, 0), (124, 25), (top - 1, 31)):
            got = b.align_dt_segmented(s_max, seg)
            assert got == [w if w[0] <= s_max else NOT_FOUND for w in want]
            check_info(b, pairs, got, cm, s_max, seg, False, False)
        assert b.align_dt_segmented(BIG, 24)[0][0] == 124 and b.dt_segmented_info()["rounds"] == top // 24 + 1 > 6
        assert b.align_dt_segmented(BIG, top + 1) == want  # a seg above every cost: one round
        info = b.dt_segmented_info()
        assert info["rounds"] == info["chunks"] == 1 and info["seg_jobs"] == len(pairs) and info["refill_cells"] > 0
        assert b.last_forward_ms > 0 and b.last_refill_ms > 0 and b.last_trace_ms > 0
    finally:
        b.close()
    # STEEP, Ew = 9 above E = 2: seventeen rounds of nine costs for a gap of 18 bytes
    b = Affine4Batch(cases.gap18(), cases.STEEP, trace=True)
    try:
        got = b.align_dt_segmented(BIG, 9)
        assert [g[0] for g in got] == [146, 146] and b.dt_segmented_info()["rounds"] == 17 and b.dt_segmented_info()["seg_jobs"] == 34
        check_info(b, cases.gap18(), got, cases.STEEP, BIG, 9, False, False)
    finally:
        b.close()


def test_any_byte_and_empty_sequences():
    pairs = ENDS["any_byte"] + [(b"\x00\xff" * 40, b"\xff\x00" * 21), (b"\x00" * 9, b"\x00" * 17), (b"", b""), (b"", b"ACGTACGTAC"),
                                (b"ACGTACGTACGTACGTACGTACGTA", b""), (b"A", b""), (b"", b"\x00")]
    for fs, fe in dt4_cases.SETTINGS:
        check_batch(pairs, MODELS["double_affine"], fs, fe, want=oracle(pairs, "double_affine", fs, fe))
    check_batch(pairs, cases.STEEP, True, True, want=oracle(pairs, "steep", True, True))


def test_the_call_leaves_the_batch_alone():
    pairs = ENDS["flanked"][::3] + ENDS["tied"] + NEW["long_gap"]
    cm = MODELS["double_affine"]
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        nw, dt = b.run().tolist(), b.run_dt(BIG).tolist()
        glob_ends = b.ends().tolist()
        ends_before = b.align_dt_ends(BIG, True, False)
        first = b.align_dt_segmented(BIG, 0, True, False)
        assert first == ends_before
        assert b.align_dt_segmented(BIG, 0, True, False) == first  # a repeated call is identical
        b.align_dt_segmented(BIG, 24)
        assert b.ends().tolist() == glob_ends
        assert b.run_dt(BIG).tolist() == dt and b.run().tolist() == nw  # the batch is still global: run_dt() does not refuse it
        assert b.align_dt_ends(BIG, True, False) == ends_before
        b.set_free_ends(True, True)
        free, free_ends = b.run().tolist(), b.ends().tolist()
        got = b.align_dt_segmented(BIG, 25)  # the call's switches (both off), not the batch's
        assert [g[0] for g in got] == dt and [g[3] for g in got] == [len(x) for x, _ in pairs] and all(g[2] == 0 for g in got)
        assert b.ends().tolist() == free_ends and b.run().tolist() == free
        with pytest.raises(ValueError, match="pa_affine4_batch_run_dt: .*ends-free"):  # the setting is still on
            b.run_dt(10)
        b.set_chain(True)  # neither read nor changed
        assert [g[0] for g in b.align_dt_segmented(BIG, 0, True, True)] == free
        assert b.chain_info()["on"] is True
    finally:
        b.close()


def test_refusals():
    pairs = GLOBAL["tails"][:5]
    L = pa.capi.load()
    fn = "pa_affine4_batch_align_dt_seg"
    none = (None,) * 7
    b = Affine4Batch(pairs, MODELS["double_affine"])  # no trace
    try:
        with pytest.raises(ValueError, match=fn + ": the batch was created without trace"):
            b.align_dt_segmented(10)
        assert L.pa_affine4_batch_align_dt_seg(b._h, 0, 0, 5, 0, *none) == -4
    finally:
        b.close()
    b = Affine4Batch(pairs, MODELS["double_affine"], trace=True)  # Ew is 24
    try:
        for seg in (1, 23):
            with pytest.raises(ValueError, match=fn + ": seg = %d .*Ew.* is 24" % seg):
                b.align_dt_segmented(10, seg)
        assert len(b.align_dt_segmented(10, 24)) == 5
        assert L.pa_affine4_batch_align_dt_seg(b._h, 0, 0, 5, 1 << 30, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "seg" in pa.capi.last_error() and "Ew" in pa.capi.last_error()
        assert L.pa_affine4_batch_align_dt_seg(b._h, 2, 0, 5, 0, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "free_start" in pa.capi.last_error()
        assert L.pa_affine4_batch_align_dt_seg(b._h, 0, -1, 5, 0, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "free_end" in pa.capi.last_error()
        assert L.pa_affine4_batch_align_dt_seg(b._h, 1, 1, -1, 0, *none) == -4
        assert pa.capi.last_error().startswith(fn + ":") and "s_max" in pa.capi.last_error()
        assert L.pa_affine4_batch_align_dt_seg(b._h, 1, 1, 5, 0, *none) == 0  # every output is optional
        assert b.dt_segmented_info()["chunks"] == 1
    finally:
        b.close()
    b = Affine4Batch(pairs, cases.STEEP, trace=True)  # E is 2, Ew is 9: a seg the main layer alone would allow is refused
    try:
        for seg in (2, 8):
            with pytest.raises(ValueError, match=fn + ": seg = %d .*Ew.* is 9" % seg):
                b.align_dt_segmented(10, seg)
        assert b.align_dt_segmented(BIG, 9) == b.align_dt_ends(BIG, False, False)
    finally:
        b.close()


def test_edge_batches():
    b = Affine4Batch([], MODELS["double_affine"], trace=True)
    try:
        assert b.align_dt_segmented(5) == [] and b.align_dt_segmented(5, 30, True, True) == []
        assert b.dt_segmented_info() == dict(chunks=0, rounds=0, seg_jobs=0, refill_cells=0, bytes_max=0)
    finally:
        b.close()
    pairs = [p for p in NEW["ladder"]]  # unequal pairs: none is found at s_max = 0
    b = Affine4Batch(pairs, MODELS["double_affine"], trace=True)
    try:
        assert b.dt_segmented_info() == dict(chunks=0, rounds=0, seg_jobs=0, refill_cells=0, bytes_max=0)  # before the first call
        assert b.align_dt_segmented(0) == [NOT_FOUND] * len(pairs)
        info = b.dt_segmented_info()
        assert info["chunks"] == 1 and info["rounds"] == 0 and info["seg_jobs"] == 0 and info["refill_cells"] == 0 and info["bytes_max"] > 0
        assert b.dt_info()["found"] == 0 and b.dt_info()["not_found"] == len(pairs)
    finally:
        b.close()


_CHILD = """
import json, sys
from astar_pairwise_aligner_amd import Affine4Batch
from tests import affine4_dt_cases as cases
name, s_max, fs = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
pairs = [(b"ACGT", b"ACG"), cases.global_cases()["mixed"][9]] if name == "mixed" else cases.ring_wraps() * 12
b = Affine4Batch(pairs, cases.DOUBLE, trace=True)
out = {}
try:
    b.align_dt_ends(s_max, fs, fs)
    out["ends_error"] = None
except ValueError as e:
    out["ends_error"] = str(e)
out["seg"] = b.align_dt_segmented(s_max, 0, fs, fs)
out["info"] = b.dt_segmented_info()
b.close()
print(json.dumps(out))
"""


def child(name, s_max, fs, budget_mb):
    env = dict(os.environ, PA_AFFINE_TRACE_BUDGET_MB=repr(budget_mb))
    r = subprocess.run([sys.executable, "-c", _CHILD, name, str(s_max), str(int(fs))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_memory_is_below_that_of_every_front():
    """A budget between the two byte figures of the 2.9 kbp pair, in a fresh child process: every front of it does not fit, its
    segments do."""
    cm = MODELS["double_affine"]
    pairs = [(b"ACGT", b"ACG"), GLOBAL["mixed"][9]]
    n, m = len(pairs[1][0]), len(pairs[1][1])
    assert n == 2900
    want = oracle(pairs, "double_affine", False, False)
    top = max(w[0] for w in want)
    lo, hi = seg_bytes(n, m, cm, top, 0, False, False), ends_bytes(n, m, cm, top, False, False)
    assert lo < hi / 4
    budget = (lo + hi) / 2
    out = child("mixed", top, False, budget / 1048576)
    assert out["ends_error"] is not None and "exceed the budget" in out["ends_error"] and "pair 1:" in out["ends_error"]
    assert [tuple(x) for x in out["seg"]] == want
    assert out["info"]["chunks"] == 1 and out["info"]["bytes_max"] == lo + seg_bytes(4, 3, cm, top, 0, False, False) <= budget


def test_small_budget_chunks_with_the_same_results():
    pairs = dt4_cases.ring_wraps() * 12
    cm = MODELS["double_affine"]
    want = oracle(pairs, "double_affine", False, False)
    s_max = max(w[0] for w in want) - 1
    exp = [w if w[0] <= s_max else NOT_FOUND for w in want]
    per_pair = [seg_bytes(len(x), len(y), cm, s_max, 0, False, False) for x, y in pairs]
    budget = max(2 * max(per_pair), sum(per_pair) // 5)  # several chunks, and room for every pair
    assert budget < sum(per_pair) / 2
    out = child("ring_wraps", s_max, False, budget / 1048576)
    assert out["ends_error"] is None
    assert [tuple(x) for x in out["seg"]] == exp
    assert out["info"]["chunks"] > 1 and out["info"]["bytes_max"] <= budget
    b = Affine4Batch(pairs, cm, trace=True)  # the default budget: one chunk
    try:
        assert b.align_dt_segmented(s_max) == exp
        info = b.dt_segmented_info()
        assert info["chunks"] == 1 and info["seg_jobs"] == out["info"]["seg_jobs"] and info["refill_cells"] == out["info"]["refill_cells"]
        assert out["info"]["rounds"] >= info["rounds"]
    finally:
        b.close()


@pytest.mark.parametrize("name", sorted(heavy.MODELS4))
def test_heavy_models(name):
    """Costs up to 1000 and Ew up to 1000 (rings and heads of a thousand rows, fronts that are empty 999 times in 1000), at seg = Ew and
    the default, against align_dt_ends of the same batch at the batch's largest cost and that minus one."""
    cm = heavy.MODELS4[name]
    assert Ew(cm) >= 800
    lists = heavy.dt4_cases()
    pairs = [p for case in sorted(lists) for p in lists[case]]
    check_batch(pairs, cm, False, False, bounds="top", segs=(Ew(cm), 0))
    check_batch(heavy.dt_planted(), cm, True, True, bounds="top", segs=(Ew(cm), 0))


@pytest.mark.parametrize("name", sorted(rnd.models4())[::4])
def test_random_models(name):
    cm = rnd.models4()[name]
    pairs = rnd.pairs_for(cm)[:8]
    check_batch(pairs, cm, False, False, segs=(Ew(cm), 0))
    check_batch(pairs, cm, True, True, segs=(Ew(cm), 0))
