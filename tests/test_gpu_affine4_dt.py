"""The diagonal-transition route of the batched double-affine aligner (Affine4Batch.run_dt / align_dt / run_dt_ends / align_dt_ends,
map_affine_dt) against the plain restatement of tests/affine4_dt_plain.py: cost, exact CIGAR string, start and end over the pairs of
tests/affine4_dt_cases.py under the three models of affine4_ends_cases.MODELS, at four values of s_max taken from the oracle (the batch's
largest cost, that minus one, the median, 0); plus the costs and ends of Affine4Batch.run() on the same batch, and what the calls must
leave alone.  The counterpart of tests/test_gpu_affine_dt.py and tests/test_gpu_affine_dt_ends.py."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch
from tests import affine4_dt_cases as cases
from tests import affine_plain as ap
from tests.affine4_dt_plain import affine4_dt, mean_w
from tests.affine4_plain import affine4_verify
from tests.affine_dt_plain import affine_dt
from tests.affine_ends_cases import MODELS as TWO_LAYER_MODELS
from tests.affine_ends_cases import mutate

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
MODELS = cases.MODELS
GLOBAL = cases.global_cases()
ENDS = cases.ends_cases_all()
BIG = (1 << 30) - 1
NOT_FOUND = (-1, "", -1, -1)
_ORACLE = {}
GLOBAL_PARAMS = [(c, n) for c in sorted(GLOBAL) for n in cases.models_of(c)]
# all four settings under double_affine, both ends free under the other two models
ENDS_PARAMS = [(c, n, s) for c in sorted(ENDS) for n in cases.models_of(c) for s in cases.SETTINGS if n == "double_affine" or s == (True, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def oracle(pairs, name, fs=False, fe=False):
    """(cost, cigar, start, end) of every pair without a bound; computed once per (pair, model, setting)."""
    out = []
    for x, y in pairs:
        key = (x, y, name, fs, fe)
        if key not in _ORACLE:
            _ORACLE[key] = affine4_dt(x, y, MODELS[name], BIG, fs, fe)
        out.append(_ORACLE[key])
    return out


def bounded(want, s_max):
    return [w if w[0] <= s_max else NOT_FOUND for w in want]


def bounds_of(want):
    """The batch's largest cost (everything found), that minus one (exactly the most expensive pairs are not), the median, and 0."""
    costs = sorted(w[0] for w in want)
    return sorted({costs[-1], max(costs[-1] - 1, 0), costs[len(costs) // 2], 0}, reverse=True)


def check_info(b, exp, npairs):
    info = b.dt_info()
    assert info["found"] == sum(w[0] >= 0 for w in exp) and info["found"] + info["not_found"] == npairs
    assert info["front_cells"] > 0 and info["chunks"] >= 1 and info["bytes_max"] > 0
    return info


def check_global_at(b, pairs, cm, want, s_max):
    exp = bounded(want, s_max)
    costs = b.run_dt(s_max)
    assert costs.dtype == np.int32 and costs.tolist() == [w[0] for w in exp], s_max
    info = check_info(b, exp, len(pairs))
    got = b.align_dt(s_max)
    assert len(got) == len(pairs)
    for p, ((x, y), e, g) in enumerate(zip(pairs, exp, got)):
        assert g == e[:2], (p, len(x), len(y), s_max)
        if g[0] >= 0:
            assert affine4_verify(g[1], x, y, cm) == g[0] and ap.no_adjacent_same_op(g[1])
    assert check_info(b, exp, len(pairs))["found"] == info["found"]


def check_global(pairs, name, cm=None, want=None):
    """Under MODELS[name] against oracle(pairs, name); or under `cm` against `want`, [(cost, CIGAR, ..)] of every pair without a bound."""
    cm = MODELS[name] if cm is None else cm
    want = oracle(pairs, name) if want is None else want
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        nw = b.run().tolist()
        assert nw == [w[0] for w in want]  # the DT cost is the NW cost of the same batch
        for s_max in bounds_of(want):
            check_global_at(b, pairs, cm, want, s_max)
        top = bounds_of(want)[0]
        assert b.run_dt(top).tolist() == nw
        first = (b.run_dt(top).tolist(), b.align_dt(top))
        assert (b.run_dt(top).tolist(), b.align_dt(top)) == first  # a repeated call gives the same answer
        assert b.run().tolist() == nw                              # run() after run_dt() is unchanged
    finally:
        b.close()


@pytest.mark.parametrize("case,name", GLOBAL_PARAMS)
def test_every_global_case_list_and_model(case, name):
    check_global(GLOBAL[case], name)


def check_ends_at(b, pairs, cm, fs, fe, want, s_max):
    exp = bounded(want, s_max)
    costs, ends = b.run_dt_ends(s_max, fs, fe)
    assert costs.dtype == np.int32 and ends.dtype == np.int64
    assert costs.tolist() == [w[0] for w in exp] and ends.tolist() == [w[3] for w in exp], s_max
    info = check_info(b, exp, len(pairs))
    got = b.align_dt_ends(s_max, fs, fe)
    assert len(got) == len(pairs)
    for p, ((x, y), e, g) in enumerate(zip(pairs, exp, got)):
        assert g == e, (p, len(x), len(y), s_max)
        if g[0] >= 0:
            assert affine4_verify(g[1], x[g[2]:g[3]], y, cm) == g[0] and ap.no_adjacent_same_op(g[1])
    assert check_info(b, exp, len(pairs))["found"] == info["found"]


def check_ends(pairs, name, fs, fe, cm=None, want=None):
    cm = MODELS[name] if cm is None else cm
    want = oracle(pairs, name, fs, fe) if want is None else want
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        for s_max in bounds_of(want):
            check_ends_at(b, pairs, cm, fs, fe, want, s_max)
        top = bounds_of(want)[0]
        first = ([r.tolist() for r in b.run_dt_ends(top, fs, fe)], b.align_dt_ends(top, fs, fe))
        assert ([r.tolist() for r in b.run_dt_ends(top, fs, fe)], b.align_dt_ends(top, fs, fe)) == first  # a repeated call is identical
        # cost and end are those of the ends-free DP of the same batch
        b.set_free_ends(fs, fe)
        assert b.run().tolist() == first[0][0] and b.ends()[:, 1].tolist() == first[0][1]
    finally:
        b.close()


@pytest.mark.parametrize("case,name,setting", ENDS_PARAMS, ids=["%s-%s-fs%d-fe%d" % (c, n, *s) for c, n, s in ENDS_PARAMS])
def test_every_ends_free_case_list_model_and_setting(case, name, setting):
    check_ends(ENDS[case], name, *setting)


def test_one_batch_in_wide_blocks_and_one_in_narrow_ones():
    """mixed has a mean W above 256 at its largest cost (four wavefronts per pair), gaps stays below at every bound (one); under
    free_start windows is wide and tied narrow.  The widths are the host's rule restated (tests/affine4_dt_plain.py mean_w)."""
    cm = MODELS["double_affine"]
    want = oracle(GLOBAL["mixed"], "double_affine")
    assert mean_w(GLOBAL["mixed"], cm, bounds_of(want)[0]) > cases.WIDE_MEAN and mean_w(GLOBAL["gaps"], cm, BIG) <= cases.WIDE_MEAN
    assert mean_w(ENDS["windows"], cm, BIG, True, True) > cases.WIDE_MEAN and mean_w(ENDS["tied"], cm, BIG, True, True) <= cases.WIDE_MEAN
    for pairs in (GLOBAL["mixed"], GLOBAL["gaps"]):
        want = oracle(pairs, "double_affine")
        b = Affine4Batch(pairs, cm)
        try:
            assert b.run_dt(BIG).tolist() == [w[0] for w in want]
        finally:
            b.close()
    # the tied ends of y * 8 across the wavefronts of a wide block: the lowest wins
    pairs = ENDS["tied"][:2] + ENDS["windows"]
    assert mean_w(pairs, cm, BIG, True, True) > cases.WIDE_MEAN
    want = oracle(pairs, "double_affine", True, True)
    b = Affine4Batch(pairs, cm)
    try:
        costs, ends = b.run_dt_ends(BIG)
        assert costs.tolist() == [w[0] for w in want] and ends.tolist() == [w[3] for w in want] and (costs[0], ends[0]) == (0, 40)
    finally:
        b.close()


def test_any_byte_and_empty_sequences():
    rng = np.random.default_rng(5)
    y = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    pairs = [(y, mutate(rng, y, 0.1, bytes(range(256)))), (b"\x00\xff" * 40, b"\xff\x00" * 21), (b"\x00" * 9, b"\x00" * 17), (b"", b""),
             (b"", b"ACGTACGTAC"), (b"ACGTACGTACGTACGTACGTACGTA", b""), (b"A", b""), (b"", b"\x00")]
    for name in sorted(MODELS):
        check_global(pairs, name)
    for fs, fe in cases.SETTINGS:
        check_ends(pairs + ENDS["any_byte"], "double_affine", fs, fe)


def test_the_calls_leave_the_batch_alone():
    pairs = ENDS["flanked"][::3] + ENDS["tied"]
    b = Affine4Batch(pairs, MODELS["double_affine"], trace=True)
    try:
        nw, dt = b.run().tolist(), b.run_dt(BIG).tolist()
        assert nw == dt
        glob_ends = b.ends().tolist()
        b.run_dt_ends(BIG)
        b.align_dt_ends(BIG, True, False)
        assert b.ends().tolist() == glob_ends                           # still the global run()'s
        assert b.run_dt(BIG).tolist() == dt and b.run().tolist() == nw  # the batch is still global: run_dt() does not refuse it
        b.set_free_ends(True, True)
        free, free_ends = b.run().tolist(), b.ends().tolist()
        costs, ends = b.run_dt_ends(BIG, False, False)                  # the call's switches, not the batch's
        assert costs.tolist() == dt and ends.tolist() == [len(x) for x, _ in pairs]
        assert b.align_dt_ends(BIG, False, False) == [w[:2] + (0, len(x)) for w, (x, _) in zip(oracle(pairs, "double_affine"), pairs)]
        assert b.ends().tolist() == free_ends and b.run().tolist() == free
        with pytest.raises(ValueError, match="pa_affine4_batch_run_dt: .*ends-free"):  # the setting is still on
            b.run_dt(10)
        with pytest.raises(ValueError, match="pa_affine4_batch_align_dt: .*ends-free"):
            b.align_dt(10)
        b.set_chain(True)  # neither read nor changed
        assert b.run_dt_ends(BIG)[0].tolist() == free and b.chain_info()["on"] is True
    finally:
        b.close()


def test_refusals():
    pairs = GLOBAL["tails"][:5]
    b = Affine4Batch(pairs, MODELS["double_affine"])  # no trace
    try:
        with pytest.raises(ValueError, match="pa_affine4_batch_align_dt: the batch was created without trace"):
            b.align_dt(10)
        with pytest.raises(ValueError, match="pa_affine4_batch_align_dt_ends: the batch was created without trace"):
            b.align_dt_ends(10)
        assert b.run_dt(1000).tolist() == b.run().tolist() and len(b.run_dt_ends(10)[0]) == 5
        L = pa.capi.load()
        assert L.pa_affine4_batch_run_dt(b._h, -1, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine4_batch_run_dt:") and "s_max" in pa.capi.last_error()
        assert L.pa_affine4_batch_run_dt_ends(b._h, 1, 1, -1, None, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine4_batch_run_dt_ends:") and "s_max" in pa.capi.last_error()
        assert L.pa_affine4_batch_run_dt_ends(b._h, 2, 0, 5, None, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine4_batch_run_dt_ends:") and "free_start" in pa.capi.last_error()
        assert L.pa_affine4_batch_align_dt_ends(b._h, 0, -1, 5, None, None, None, None, None, None) == -4
        assert pa.capi.last_error().startswith("pa_affine4_batch_align_dt_ends:") and "free_end" in pa.capi.last_error()
        assert L.pa_affine4_batch_run_dt(b._h, 5, None, None) == 0 and L.pa_affine4_batch_run_dt_ends(b._h, 1, 1, 5, None, None, None) == 0
        b.set_free_ends(False, True)
        with pytest.raises(ValueError, match="pa_affine4_batch_run_dt: .*ends-free"):
            b.run_dt(10)
    finally:
        b.close()


def test_empty_batch():
    b = Affine4Batch([], MODELS["double_affine"], trace=True)
    try:
        assert b.run_dt(5).tolist() == [] and b.align_dt(5) == []
        costs, ends = b.run_dt_ends(5)
        assert costs.tolist() == [] and ends.tolist() == [] and b.align_dt_ends(5) == []
        assert b.dt_info() == dict(found=0, not_found=0, chunks=0, front_cells=0, extend_chars=0, bytes_max=0)
    finally:
        b.close()
    assert pa.map_affine_dt([], MODELS["double_affine"], 3) == []


def test_map_affine_dt_on_two_and_four_layers():
    pairs = ENDS["packed_unequal"] + ENDS["tied"]
    want = oracle(pairs, "double_affine", True, True)
    K = bounds_of(want)[1]  # the largest cost minus one
    assert pa.map_affine_dt(pairs, MODELS["double_affine"], K) == bounded(want, K)
    assert pa.map_affine_dt(pairs, MODELS["double_affine"], BIG, free_start=False) == oracle(pairs, "double_affine", False, True)
    # cost and end (not start and CIGAR, which may be another optimal placement) are those of the DP route
    assert [(c, e) for c, _, _, e in pa.map_affine_dt(pairs, MODELS["double_affine"], BIG)] == [(c, e) for c, _, _, e in pa.map_affine(pairs, MODELS["double_affine"])]
    two = TWO_LAYER_MODELS["affine"]
    assert pa.map_affine_dt(pairs, two, 40) == pa.map_affine(pairs, two, s_max=40)
    assert pa.map_affine_dt(pairs, two, BIG, False, False) == [(c, g, 0, len(x)) for (c, g), (x, _) in zip((affine_dt(x, y, two, BIG) for x, y in pairs), pairs)]


_CHILD = """
import json, sys
from astar_pairwise_aligner_amd import Affine4Batch
from tests import affine4_dt_cases as cases
pairs = cases.ring_wraps() * 12
s_max = int(sys.argv[1])
b = Affine4Batch(pairs, cases.DOUBLE, trace=True)
out = {"run": b.run_dt(s_max).tolist(), "run_info": b.dt_info()}
out["align"] = b.align_dt(s_max)
out["align_info"] = b.dt_info()
b.close()
big = [(b"ACGT", b"ACG"), cases.global_cases()["mixed"][9]]
b = Affine4Batch(big, cases.DOUBLE, trace=True)
try:
    b.align_dt(1 << 20)
    out["refused"] = None
except ValueError as e:
    out["refused"] = str(e)
out["big_run"] = b.run_dt(1 << 20).tolist()
b.close()
print(json.dumps(out))
"""


def test_small_budget_chunks_and_refuses():
    """PA_AFFINE_TRACE_BUDGET_MB = 1 in a fresh child process: the rings of 72 pairs (36 rows of W values each, 1.6 MB in all) take two
    chunks, their traced fronts (0.5 to 0.7 MB each) a chunk each, with the results of the default budget; the traced fronts of a
    2.9 kbp pair under a loose bound (hundreds of megabytes) alone exceed it, and the call names the pair, while its rings (0.8 MB) fit."""
    pairs = cases.ring_wraps() * 12
    want = oracle(pairs, "double_affine")
    s_max = max(w[0] for w in want) - 1
    env = dict(os.environ, PA_AFFINE_TRACE_BUDGET_MB="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(s_max)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    exp = bounded(want, s_max)
    assert out["run"] == [w[0] for w in exp] and [tuple(x) for x in out["align"]] == [w[:2] for w in exp]
    assert out["run_info"]["chunks"] == 2 and out["run_info"]["bytes_max"] <= 1 << 20
    assert out["align_info"]["chunks"] == len(pairs) and out["align_info"]["bytes_max"] <= 1 << 20
    assert out["run_info"]["found"] + out["run_info"]["not_found"] == len(pairs) and out["run_info"]["not_found"] == 12
    assert out["refused"] and "pa_affine4_batch_align_dt: pair 1:" in out["refused"] and "budget" in out["refused"]
    big = [(b"ACGT", b"ACG"), GLOBAL["mixed"][9]]
    assert out["big_run"] == [w[0] for w in oracle(big, "double_affine")]  # the rings of the same pair fit
    b = Affine4Batch(pairs, MODELS["double_affine"], trace=True)  # the default budget: one chunk
    try:
        assert b.run_dt(s_max).tolist() == out["run"] and b.dt_info()["chunks"] == 1
        assert b.dt_info()["front_cells"] == out["run_info"]["front_cells"] and b.dt_info()["extend_chars"] == out["run_info"]["extend_chars"]
        assert b.align_dt(s_max) == [w[:2] for w in exp]
    finally:
        b.close()
