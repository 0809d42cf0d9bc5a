"""The rectangle operator (pa_bp_profile_build, pa_bp_compute, pa_bp_fill) and the device-resident handle (pa_bp_ctx_*) against the
plain DP of tests/rect_plain.py, bit for bit, at the shapes where the routes of HipBackend::launch_rect change: the half-wave
threshold (16 words), one strip (32 words), the mailbox fill's limits (1 MiB of `values`, 64 strips), the staged route (more than
1024 strips, or PA_ENGINE_NO_FAST_PATH), unaligned column and word offsets, empty ranges, and the stored h row under every mode.

The operator calls are not compared with oracle/: tests/test_rect_plain.py pins the plain model to it on the CPU.  Only the engine
calls of the staged route (ENGINE_PAIRS) are, as everywhere else, checked against the engine over the CPU oracle kernels."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest

from tests import rect_plain as rp
from tests import strip_plain as sp
from tests.util_seq import gen_pair, mutate, rand_seq

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
FILL = "fill"


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


def _deltas(rng, k: int, kind: str) -> np.ndarray:
    return rng.integers(-1, 2, k).astype(np.int64) if kind == "random" else np.ones(k, np.int64)


def _similar_pair(n: int, m: int, seed: int):
    """`b` is two mutated copies of `a` cut to m rows: diagonals of matches all over the rectangle, not only random cells."""
    a = rand_seq(n, seed=seed)
    b = (mutate(a, 0.1, seed + 1) + mutate(a, 0.25, seed + 2) + rand_seq(m, seed=seed + 3))[:m]
    return a, b


# ---- (a) pa_bp_profile_build -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_profile_build(pa, n, m):
    a, b = rand_seq(n, seed=n), rand_seq(m, seed=m + 1)
    a2, b2 = pa.profile_build(a, b)
    assert a2.shape == (n, 2) and np.array_equal(a2, rp.a_bits(a))
    assert b2.shape == ((m + 63) // 64, 2) and np.array_equal(b2, sp.profile_words(b))


def test_profile_build_one_side_empty(pa):
    a, b = rand_seq(33, seed=1), rand_seq(130, seed=2)
    a2, b2 = pa.profile_build(b"", b)
    assert a2.shape == (0, 2) and np.array_equal(b2, sp.profile_words(b))
    a2, b2 = pa.profile_build(a, b"")
    assert b2.shape == (0, 2) and np.array_equal(a2, rp.a_bits(a))


# ---- (b) pa_bp_compute -------------------------------------------------------------------------------------------------------

# words: the half-wave threshold (16), one strip exactly (32), strip boundaries with a half-wave (33, 48, 65), a partial (49, 63,
# 97, 129) and a full (64, 96) last strip
COMPUTE_WS = [1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 96, 97, 129]
_N_SHORT, _N_EDGE, _N_LONG = [1, 2, 31, 32], [33, 63, 64, 65], [255, 256, 257, 1000]
# every w meets a short, a chunk-edge and a long n; the rotation makes every n meet several w
COMPUTE_SHAPES = [(ns[(k + r) % 4], w) for k, w in enumerate(COMPUTE_WS) for r, ns in enumerate((_N_SHORT, _N_EDGE, _N_LONG))]


@pytest.mark.parametrize("n,w", COMPUTE_SHAPES)
def test_compute(pa, n, w):
    """Sum, v2 and (exact) h2 against the plain DP; exact_end == 0 takes the padded-tail chunk variants and must leave h2 as it was
    (include/pa_bitpacking_hip.h) while the sum and v2 stay exact."""
    rng = np.random.default_rng(n * 1000 + w)
    for ragged in (False, True):
        m = 64 * w - (int(rng.integers(1, 64)) if ragged else 0)
        a, b = _similar_pair(n, m, seed=n * 7 + w + ragged)
        a2, b2 = rp.a_bits(a), sp.profile_words(b)
        for kind in ("random", "ones"):
            top, left = _deltas(rng, n, kind), _deltas(rng, 64 * w, kind)
            s, right, bottom = rp.rect(a, b, 0, n, 0, w, top, left)
            for exact in (True, False):
                h2, v2 = rp.h_words(top), sp.v_words(left)
                got = pa.compute(a2, b2, h2, v2, exact)
                what = (n, w, m, kind, exact)
                assert got == s, what
                assert np.array_equal(v2, sp.v_words(right)), what
                assert np.array_equal(h2, rp.h_words(bottom if exact else top)), what


@pytest.mark.parametrize("exact", [True, False])
def test_compute_without_columns_or_rows(pa, exact):
    rng = np.random.default_rng(3)
    a, b = rand_seq(50, seed=5), rand_seq(64 * 3 - 9, seed=6)
    a2, b2 = rp.a_bits(a), sp.profile_words(b)
    top, left = _deltas(rng, 50, "random"), _deltas(rng, 192, "random")
    v2 = sp.v_words(left)
    assert pa.compute(a2[:0], b2, np.zeros((0, 2), np.uint64), v2, exact) == 0  # n == 0
    assert np.array_equal(v2, sp.v_words(left))
    h2 = rp.h_words(top)
    assert pa.compute(a2, b2[:0], h2, np.zeros((0, 2), np.uint64), exact) == int(top.sum())  # w == 0: the bottom row is the top row
    assert np.array_equal(h2, rp.h_words(top))


# ---- (c) pa_bp_fill ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("w", [16, 17, 32, 33, 65])
@pytest.mark.parametrize("n", [1, 33, 256, 300])
def test_fill(pa, n, w):
    rng = np.random.default_rng(n * 100 + w)
    a, b = _similar_pair(n, 64 * w - int(rng.integers(0, 64)), seed=n + w)
    top, left = _deltas(rng, n, "random"), _deltas(rng, 64 * w, "random")
    s, right, bottom, cols = rp.rect_columns(a, b, 0, n, 0, w, top, left)
    h2, v2 = rp.h_words(top), sp.v_words(left)
    got, values = pa.fill(rp.a_bits(a), sp.profile_words(b), h2, v2)
    assert got == s
    assert np.array_equal(v2, sp.v_words(right)) and np.array_equal(h2, rp.h_words(bottom))
    assert np.array_equal(values, rp.values_words(cols))


# ---- the handle against HandleModel ------------------------------------------------------------------------------------------


def call_name(call) -> str:
    kind, i0, i1, w0, w1 = call
    return f"{'fill' if kind == FILL else rp.MODE_NAMES[kind]}(i0={i0}, i1={i1}, w0={w0}, w1={w1})"


def play(ctx, model, call, rng, where=""):
    """One call with a random left column on the handle and on the model; everything either returns must agree."""
    kind, i0, i1, w0, w1 = call
    v = rp.rand_v(rng, w1 - w0)
    vg = v.copy()
    what = f"{where}{call_name(call)}"
    if kind == FILL:
        values, hb = ctx.fill(i0, i1, w0, w1, vg)
        want_values, want_hb, want_v = model.fill(i0, i1, w0, w1, v)
        assert np.array_equal(hb.astype(np.int64), want_hb), f"{what}: h_bottom"
        bad = np.argwhere(values != want_values)
        assert len(bad) == 0, f"{what}: values differ at {len(bad)} places, first (column, word, plane) = {bad[0].tolist()}"
    else:
        got = ctx.compute(i0, i1, w0, w1, vg, kind)
        want, want_v = model.compute(i0, i1, w0, w1, v, kind)
        assert got == want, f"{what}: sum {got}, plain DP {want}"
    bad = np.argwhere(vg != want_v)
    assert len(bad) == 0, f"{what}: v differs in {len(bad)} places, first (word, plane) = {bad[0].tolist()}"


GRID_I0 = [0, 1, 15, 16, 17, 31, 32, 33, 255, 257]
GRID_N = [1, 31, 32, 33, 64, 300]


def grid_ranges(W: int):
    return [(0, 1), (0, 16), (0, 17), (3, 19), (5, 37), (16, 48), (31, 33), (0, W), (W - 1, W)]


def grid_check(pa, a, b, i0s, ns, w0, w1, seed):
    """Every mode at every (i0, n), and the ranges that end at |a|.  First pass: Input over the never-written row (all zeros; Input
    stores nothing, so it stays that way).  Second pass: Output writes the stored row over exactly these columns, Input reads it,
    Update reads and rewrites it, Input reads that, None ignores it."""
    rng = np.random.default_rng(seed)
    ctx, model = pa.OperatorContext(a, b), rp.HandleModel(a, b)
    cols = [(i0, i0 + n) for i0 in i0s for n in ns] + [(len(a) - n, len(a)) for n in ns]
    try:
        for i0, i1 in cols:
            play(ctx, model, (rp.H_INPUT, i0, i1, w0, w1), rng, "zero row: ")
        assert not model.h.any()
        for i0, i1 in cols:
            for mode in (rp.H_OUTPUT, rp.H_INPUT, rp.H_UPDATE, rp.H_INPUT, rp.H_NONE):
                play(ctx, model, (mode, i0, i1, w0, w1), rng)
    finally:
        ctx.close()


GRID_PAIR = (3001, 64 * 94 - 21)  # about 3000 x 6000, |b| ragged


@pytest.mark.parametrize("r", range(9))
def test_handle_offsets_grid(pa, r):
    a, b = _similar_pair(*GRID_PAIR, seed=77)
    w0, w1 = grid_ranges((len(b) + 63) // 64)[r]
    grid_check(pa, a, b, GRID_I0, GRID_N, w0, w1, seed=r)


def random_call(rng, n_a: int, W: int, max_n: int, max_w: int):
    kind = [rp.H_NONE, rp.H_INPUT, rp.H_UPDATE, rp.H_OUTPUT, FILL][int(rng.choice(5, p=[0.15, 0.3, 0.2, 0.2, 0.15]))]
    n = 0 if rng.random() < 0.04 else int(rng.integers(1, max_n + 1))
    if kind == FILL:
        n = min(n, 60)
    w = 0 if rng.random() < 0.08 else int(rng.integers(1, max_w + 1))
    i0, w0 = int(rng.integers(0, n_a - n + 1)), int(rng.integers(0, W - w + 1))
    return kind, i0, i0 + n, w0, w0 + w


def script_check(pa, seed: int, ncalls: int, n_a: int = 2000, m: int = 64 * 70 - 37, max_n: int = 400, max_w: int = 70):
    """A random script on a fresh handle and the model in lockstep.  Replay one alone with script_check(pa, seed, k + 1)."""
    rng = np.random.default_rng(seed)
    a, b = _similar_pair(n_a, m, seed=1000 + seed)
    ctx, model = pa.OperatorContext(a, b), rp.HandleModel(a, b)
    try:
        for k in range(ncalls):
            call = random_call(rng, n_a, model.words, max_n, max_w)
            play(ctx, model, call, rng, f"seed {seed}, call {k}: ")
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", range(4))
def test_handle_random_scripts(pa, seed):
    script_check(pa, seed, 150 + 50 * seed)


def fill_check(pa, a, b, cases, seed):
    """Fills element by element; an Input over the same columns before and after shows that the stored row did not change."""
    rng = np.random.default_rng(seed)
    ctx, model = pa.OperatorContext(a, b), rp.HandleModel(a, b)
    try:
        play(ctx, model, (rp.H_OUTPUT, 0, len(a), 0, 2), rng, "stored row: ")
        assert model.h.any()
        for i0, i1, w0, w1 in cases:
            before = model.h.copy()
            play(ctx, model, (rp.H_INPUT, i0, i1, 1, 3), rng, "before the fill: ")
            play(ctx, model, (FILL, i0, i1, w0, w1), rng)
            assert np.array_equal(model.h, before)
            play(ctx, model, (rp.H_INPUT, i0, i1, 1, 3), rng, f"after {call_name((FILL, i0, i1, w0, w1))}: ")
    finally:
        ctx.close()


FILL_PAIR = (601, 64 * 330 - 17)


@pytest.mark.parametrize("w", [1, 16, 17, 32, 33, 40, 64, 65])
def test_handle_fill_word_offsets(pa, w):
    a, b = _similar_pair(*FILL_PAIR, seed=5)
    fill_check(pa, a, b, [(17, 17 + 70, 3, 3 + w), (255, 255 + 33, 31, 31 + w), (1, 2, 7, 7 + w), (601 - 31, 601, 330 - w, 330)], seed=w)


@pytest.mark.parametrize("n,w", [(256, 256), (255, 257), (257, 255), (256, 257), (257, 256)])
def test_handle_fill_around_one_mib(pa, n, w):
    """16 n w bytes of `values` against 1 MiB: 256 x 256 words is exactly 1 MiB and 255 x 257 just under it, both still through the
    mailbox; 256 x 257 and 257 x 256 are above it and take the staged route."""
    assert 256 * 256 * 16 == 1 << 20
    a, b = _similar_pair(*FILL_PAIR, seed=6)
    fill_check(pa, a, b, [(33, 33 + n, 5, 5 + w)], seed=n + w)


@pytest.fixture(scope="module")
def tall(pa):
    """A short `a` against a `b` of just over 32 768 words: more than 1024 strips in one rectangle."""
    a = rand_seq(53, seed=8)
    b = rand_seq(64 * (32768 + 6) - 29, seed=9)
    ctx, model = pa.OperatorContext(a, b), rp.HandleModel(a, b)
    yield ctx, model
    ctx.close()


def test_handle_fill_more_than_64_strips(tall):
    """65 strips at three columns: far below 1 MiB of `values`, and still the staged route."""
    ctx, model = tall
    rng = np.random.default_rng(11)
    play(ctx, model, (rp.H_OUTPUT, 0, 53, 0, 1), rng)
    play(ctx, model, (FILL, 17, 20, 5, 5 + 64 * 32 + 1), rng)
    play(ctx, model, (FILL, 17, 20, 5, 5 + 64 * 32), rng)  # 64 strips: the mailbox
    play(ctx, model, (rp.H_INPUT, 0, 53, 1, 2), rng, "after the fills: ")


def test_handle_staged_by_size(tall):
    """More than 1024 strips leaves the mailbox route for cost-only rectangles too.  None and Output have the same +1 top row: with the
    same left column both must return what the plain DP returns once; the row Output stored is then read back by an Input."""
    ctx, model = tall
    W = model.words
    assert (W + 31) // 32 > 1024
    rng = np.random.default_rng(12)
    v = rp.rand_v(rng, W)
    want, want_v = model.compute(1, 53, 0, W, v, rp.H_OUTPUT)
    for mode in (rp.H_NONE, rp.H_OUTPUT):
        vg = v.copy()
        assert ctx.compute(1, 53, 0, W, vg, mode) == want, rp.MODE_NAMES[mode]
        assert np.array_equal(vg, want_v), rp.MODE_NAMES[mode]
    play(ctx, model, (rp.H_INPUT, 0, 53, 2, 4), rng, "the row the staged Output stored: ")


# ---- (h) the staged route at small shapes ------------------------------------------------------------------------------------


ENGINE_PAIRS = [(300, 0.1), (3000, 0.1), (12000, 0.1)]


def engine_over_operators(pa):
    """[cost, CIGAR, statistics] of pa_align, traced, with the `incremental_doubling` configuration of tests/test_gpu_engine.py: the
    host-driven engine, whose blocks go through HipBackend::compute_chain -- one fused launch through the mailbox, or, when there is
    no mailbox route, one compute() per segment."""
    import oracle
    from tests.test_engine_cpu import configs
    from tests.test_gpu_engine import STAT_KEYS, gpu_params

    al = gpu_params(pa, configs(oracle)["incremental_doubling"]).make_aligner(True)
    out = []
    for n, e in ENGINE_PAIRS:
        a, b = gen_pair(n, e, seed=n)
        cost, cigar, stats = al.align_with_stats(a, b)
        out.append([int(cost), cigar, {k: int(stats[k]) for k in STAT_KEYS}])
    return out


def staged_child():
    """Runs in a process of its own with PA_ENGINE_NO_FAST_PATH set (the library reads it once per process): reduced forms of the
    grid, the random scripts and the fills, all through plan_rect + strip_kernel; then the engine over the same route."""
    import astar_pairwise_aligner_amd as pa

    assert os.environ.get("PA_ENGINE_NO_FAST_PATH") == "1"
    pa.require_gpu()
    a, b = _similar_pair(*GRID_PAIR, seed=77)
    for r, (w0, w1) in enumerate(grid_ranges((len(b) + 63) // 64)):
        if r in (0, 3, 4, 6, 7, 8):
            grid_check(pa, a, b, [1, 17, 33], [1, 33, 300], w0, w1, seed=100 + r)
    script_check(pa, 50, 150)
    a, b = _similar_pair(*FILL_PAIR, seed=5)
    fill_check(pa, a, b, [(17, 17 + 70, 3, 3 + w) for w in (1, 16, 17, 33, 65)] + [(255, 255 + 33, 31, 31 + 40), (1, 2, 7, 8)], seed=60)
    print("staged engine " + json.dumps(engine_over_operators(pa)))
    print("staged ok")


def test_staged_route_at_small_shapes(pa, oracle):
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from tests.test_gpu_operator_edges import staged_child
        staged_child()
    """) % str(ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PA_ENGINE_NO_FAST_PATH="1"))
    assert r.returncode == 0 and "staged ok" in r.stdout, f"child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    # the engine's chained blocks: one compute() per segment in the child, the fused chain in this process, the CPU-kernel engine
    from tests.test_engine_cpu import configs
    from tests.test_gpu_engine import STAT_KEYS

    assert "PA_ENGINE_NO_FAST_PATH" not in os.environ
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("staged engine ")]
    assert len(lines) == 1, r.stdout[-2000:]
    staged = json.loads(lines[0][len("staged engine "):])
    fused = engine_over_operators(pa)
    assert len(staged) == len(fused) == len(ENGINE_PAIRS)
    for (n, e), got_staged, got_fused in zip(ENGINE_PAIRS, staged, fused):
        a, b = gen_pair(n, e, seed=n)
        wc, wg, ws = oracle.cpu_align(a, b, configs(oracle)["incremental_doubling"])
        want = [wc, wg, {k: int(ws[k]) for k in STAT_KEYS}]
        assert got_staged == want, ("staged", n)
        assert got_fused == want, ("fused", n)


# ---- (i) argument errors -----------------------------------------------------------------------------------------------------


def test_handle_argument_errors(pa):
    a, b = _similar_pair(300, 64 * 9 - 5, seed=13)
    ctx, model = pa.OperatorContext(a, b), rp.HandleModel(a, b)
    L = pa.capi.load()
    rng = np.random.default_rng(14)
    v = rp.rand_v(rng, 16)
    values, hb, s = np.zeros((300, 16, 2), np.uint64), np.zeros(300, np.int8), C.c_int32(0)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    bad_compute = [(0, 301, 0, 9, 0), (10, 9, 0, 9, 0), (0, 300, 0, 10, 0), (0, 300, 5, 4, 0), (0, 300, 0, 9, 4)]
    bad_fill = [(0, 301, 0, 9, values), (10, 9, 0, 9, values), (0, 300, 0, 10, values), (0, 300, 5, 4, values), (0, 300, 0, 9, None)]
    try:
        play(ctx, model, (rp.H_OUTPUT, 0, 300, 0, 4), rng)
        for (i0, i1, w0, w1, mode), (f0, f1, fw0, fw1, vals) in zip(bad_compute, bad_fill):
            vg = v.copy()
            assert L.pa_bp_ctx_compute(ctx._h, i0, i1, w0, w1, p(vg), mode, C.byref(s)) == PA_E_ARG, (i0, i1, w0, w1, mode)
            assert L.pa_bp_ctx_fill(ctx._h, f0, f1, fw0, fw1, p(vg), p(vals) if vals is not None else None, p(hb)) == PA_E_ARG, (f0, f1, fw0, fw1)
            assert np.array_equal(vg, v)
            # the handle is still usable, and its stored row is what it was
            play(ctx, model, (rp.H_UPDATE, 3, 290, 2, 9), rng, "after a refused call: ")
            play(ctx, model, (FILL, 7, 40, 1, 8), rng, "after a refused call: ")
            play(ctx, model, (rp.H_INPUT, 0, 300, 0, 9), rng, "after a refused call: ")
    finally:
        ctx.close()
