"""The strips of the batched A*PA2 band search against the plain rectangle DP of tests/strip_plain.py, driven directly through
pa_debug_strip (capi.strip_probe) at their shape edges.

Paths (each with the template arguments production uses):
* dual: two jobs fused in one wavefront (run_strip_dual<false> of `simple`, run_strip_dual<true> of `full`), each job in
  either half, next to partners of other shapes;
* single: run_strip<1, .., HALF, NOPASS> (`simple`), and the TAP strips of `full`: half wave, K = 1 full wave, K = 2;
* rdv: 2 to 4 wavefronts of one workgroup meet through rdv_strip, whoever takes whom.

Every call runs twice.  v and hout carry poison around the strip, so every word or byte the strip must not write is checked
unchanged (the plain DP copies them through), and with `values` the strip's own words of v hold deltas that would change the
answer.  The dual and rdv paths also prove that dual_ok accepts each job: pa_debug_strip refuses a job production would not fuse.
"""
import numpy as np
import pytest

from tests import strip_plain as sp
from tests.util_seq import rand_seq

pytestmark = pytest.mark.gpu

BIG_PATIENCE = 20_000_000  # 0.2 s of the 100 MHz clock: a strip takes microseconds
WINDOWS = ["above", "top", "bottom", "contains", "below", "empty"]


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


def _deltas(rng, k, kind):
    if kind == "random":
        return rng.integers(-1, 2, k)
    return np.full(k, {"plus": 1, "minus": -1, "zero": 0}[kind], np.int64)


def _window(kind, word0, W):
    return {"above": (max(0, word0 - 2), word0), "top": (max(0, word0 - 1), word0 + max(1, W // 2)), "bottom": (word0 + W - 1, word0 + W + 1),
            "contains": (max(0, word0 - 1), word0 + W + 1), "below": (word0 + W, word0 + W + 2), "empty": (word0, word0)}[kind]


def make_job(rng, a, b, col0, n, word0, nlanes, *, top="random", left="random", hin=True, tap=-1, window=None, update=False):
    """A strip job with poison around it: random garbage in every v word and hout / hin byte outside the strip."""
    nwb = (len(b) + 63) // 64
    W = nlanes // 2
    v = rng.integers(0, 2**63, (nwb, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nwb, 2), dtype=np.uint64)
    v[word0 : word0 + W] = sp.v_words(_deltas(rng, 64 * W, left))
    hout = rng.integers(0, 256, len(a), dtype=np.uint8)
    job = dict(a=a, b=b, col0=col0, n=n, word0=word0, nlanes=nlanes, v=v, hout=hout, tap=tap)
    topb = sp.h_bytes(_deltas(rng, n, top))
    if update:
        hout[col0 : col0 + n] = topb
        job["hin_is_hout"] = 1
    elif hin:
        h = rng.integers(0, 256, len(a), dtype=np.uint8)
        h[col0 : col0 + n] = topb
        job["hin"] = h
    if window is not None:
        fw0, fw1 = _window(window, word0, W) if isinstance(window, str) else window
        values = rng.integers(0, 2**63, (nwb, 2), dtype=np.uint64)
        values[word0 : word0 + W] = sp.v_words(_deltas(rng, 64 * W, left))
        v[word0 : word0 + W] = sp.v_words(rng.integers(-1, 2, 64 * W))  # deltas the strip must not read
        job.update(values=values, fill_word0=fw0, fill_stride=fw1)
    return job


def _same(got, want, what):
    assert got["sum"] == want["sum"], (what, got["sum"], want["sum"])
    assert np.array_equal(got["v"], want["v"]), (what, np.flatnonzero((got["v"] != want["v"]).any(axis=1)))
    assert np.array_equal(got["hout"], want["hout"]), (what, np.flatnonzero(got["hout"] != want["hout"]))


def run(pa, mode, variant, jobs, wants, what, nwaves=0, patience=0):
    """One probe call, twice; every job's outputs equal its plain DP.  Returns the rendezvous counters of both runs."""
    cnts = []
    for rep in range(2):
        outs, cnt = pa.capi.strip_probe(mode, variant, jobs, nwaves=nwaves, patience=patience)
        for t, (o, w) in enumerate(zip(outs, wants)):
            _same(o, w, (what, mode, variant, rep, t, {k: jobs[t][k] for k in ("col0", "n", "word0", "nlanes", "tap")}))
        cnts.append(cnt)
    return cnts


def all_paths(pa, pairs, tap_variant, what, rdv_every=1):
    """Every path that accepts the jobs: the dual with each job in both halves, every single strip, the rendezvous (on every
    rdv_every-th pair)."""
    dual = [j for p in pairs for j in p]
    swapped = [j for p in pairs for j in (p[1], p[0])]
    want = {id(j): sp.strip(j, 1, tap_variant) for j in dual}
    v = 1 if tap_variant else 0
    run(pa, pa.capi.STRIP_DUAL, v, dual, [want[id(j)] for j in dual], what)
    run(pa, pa.capi.STRIP_DUAL, v, swapped, [want[id(j)] for j in swapped], what)
    singles = [1, 2] if tap_variant else [0, 1, 2]
    for var in singles:
        run(pa, pa.capi.STRIP_SINGLE, var, dual, [want[id(j)] for j in dual], what)
    # K = 2: 64-row lanes; a K = 1 tap t (odd) is the K = 2 tap (t - 1) / 2 (the same row); even taps have no K = 2 counterpart
    k1 = [j for j in dual if j["tap"] < 0 or j["tap"] % 2 == 1]
    if k1:
        k2 = [dict(j, tap=(j["tap"] - 1) // 2 if j["tap"] >= 0 else -1) for j in k1]
        run(pa, pa.capi.STRIP_SINGLE, 3, k2, [want[id(j)] for j in k1], what)
    sub = [j for p in pairs[::rdv_every] for j in p]
    for pat in (0, BIG_PATIENCE):
        for took, served, alone, _ in run(pa, pa.capi.STRIP_RDV, v, sub, [want[id(j)] for j in sub], what, nwaves=2, patience=pat):
            assert took == served and took + served + alone == len(sub), (took, served, alone)
            if pat:
                assert took == len(sub) // 2


def _seqs(rng, la, lb, seed):
    return rand_seq(la, seed=seed), rand_seq(lb, seed=seed + 1)


# ---- column edges ---------------------------------------------------------------------------------------------------------------
NS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257]


@pytest.mark.parametrize("tap_variant", [False, True])
def test_column_edges(pa, tap_variant):
    rng = np.random.default_rng(1 + tap_variant)
    jobs = []
    for i, n in enumerate(NS):
        for r in range(16):
            col0 = 16 * int(rng.integers(0, 4)) + r
            tail = (i + r) % 3 == 0  # col0 + n == |a|: the last code word is the last word of a (load_codes' clamp)
            a, b = _seqs(rng, col0 + n + (0 if tail else int(rng.integers(1, 40))), int(rng.integers(200, 700)), 7 * len(jobs))
            nlanes = 2 * int(rng.integers(1, min(16, len(b) // 64 + 1) + 1))
            nlanes = min(nlanes, 2 * ((len(b) + 63) // 64))
            tap = int(rng.integers(-1, nlanes)) if tap_variant else -1
            jobs.append(make_job(rng, a, b, col0, n, 0, nlanes, tap=tap))
    if len(jobs) % 2:
        jobs.append(jobs[0])
    all_paths(pa, list(zip(jobs[0::2], jobs[1::2])), tap_variant, "column edges")


# ---- row edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap_variant", [False, True])
def test_row_edges(pa, tap_variant):
    rng = np.random.default_rng(3 + tap_variant)
    jobs = []
    for nlanes in range(2, 33, 2):
        W = nlanes // 2
        for where in ("first", "second", "last"):
            for ragged in (0, 1, 37, 63):  # |b| mod 64: 0, or a padded last word the strip ends in
                nwb = W + 1 + int(rng.integers(0, 3))
                lb = 64 * nwb - (64 - ragged if ragged else 0)
                word0 = {"first": 0, "second": 1, "last": nwb - W}[where]
                a, b = _seqs(rng, int(rng.integers(40, 200)), lb, 11 * len(jobs))
                n = int(rng.integers(1, len(a) + 1))
                col0 = int(rng.integers(0, len(a) - n + 1))
                tap = int(rng.integers(-1, nlanes)) if tap_variant else -1
                jobs.append(make_job(rng, a, b, col0, n, word0, nlanes, tap=tap))
    all_paths(pa, list(zip(jobs[0::2], jobs[1::2])), tap_variant, "row edges")


# ---- asymmetric pairs in the dual -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap_variant", [False, True])
def test_asymmetric_pairs(pa, tap_variant):
    rng = np.random.default_rng(5 + tap_variant)
    pairs = []
    for n0 in (1, 31, 32, 33, 64, 256, 300):
        for n1 in (1, 31, 32, 33, 64, 256, 300):
            for l0 in (2, 16, 30, 32):
                for l1 in (2, 16, 30, 32):
                    p = []
                    for n, nl in ((n0, l0), (n1, l1)):
                        a, b = _seqs(rng, n + int(rng.integers(0, 50)), 32 * nl + int(rng.integers(1, 300)), int(rng.integers(0, 1 << 30)))
                        nwb = (len(b) + 63) // 64
                        col0 = int(rng.integers(0, len(a) - n + 1))
                        word0 = int(rng.integers(0, nwb - nl // 2 + 1))
                        tap = int(rng.integers(-1, nl)) if tap_variant else -1
                        p.append(make_job(rng, a, b, col0, n, word0, nl, tap=tap, hin=bool(rng.integers(0, 2))))
                    pairs.append(tuple(p))
    all_paths(pa, pairs, tap_variant, "asymmetric pairs", rdv_every=7)


# ---- boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap_variant", [False, True])
def test_boundaries(pa, tap_variant):
    rng = np.random.default_rng(7 + tap_variant)
    kinds = ["plus", "minus", "zero", "random"]
    pairs = []
    for top in kinds:
        for left in kinds:
            for hin0, hin1 in ((False, False), (True, True), (True, False), (False, True)):
                p = []
                for hin in (hin0, hin1):
                    a, b = _seqs(rng, int(rng.integers(1, 300)), int(rng.integers(64, 1100)), int(rng.integers(0, 1 << 30)))
                    nwb = (len(b) + 63) // 64
                    nl = 2 * int(rng.integers(1, min(16, nwb) + 1))
                    n = int(rng.integers(1, len(a) + 1))
                    tap = int(rng.integers(-1, nl)) if tap_variant else -1
                    p.append(make_job(rng, a, b, int(rng.integers(0, len(a) - n + 1)), n, int(rng.integers(0, nwb - nl // 2 + 1)), nl, top=top, left=left,
                                      hin=hin, tap=tap))
                pairs.append(tuple(p))
    all_paths(pa, pairs, tap_variant, "boundaries")


# ---- TAP: every tap lane in each half, values windows, the Update pattern -------------------------------------------------------
def test_tap_lanes(pa):
    rng = np.random.default_rng(9)
    pairs = []
    for nl0, nl1 in ((32, 32), (32, 6), (10, 32), (2, 20)):
        for t0 in range(-1, nl0):
            t1 = int(rng.integers(-1, nl1)) if t0 % 3 else (t0 if t0 < nl1 else -1)
            p = []
            for nl, tap in ((nl0, t0), (nl1, t1)):
                a, b = _seqs(rng, int(rng.integers(1, 280)), 32 * nl + int(rng.integers(0, 200)), int(rng.integers(0, 1 << 30)))
                n = int(rng.integers(1, len(a) + 1))
                p.append(make_job(rng, a, b, int(rng.integers(0, len(a) - n + 1)), n, 0, nl, tap=tap, update=bool(rng.integers(0, 2))))
            pairs.append(tuple(p))
    # and the other lane of the pair at every tap lane too
    pairs += [(q, p) for p, q in pairs[::3]]
    all_paths(pa, pairs, True, "tap lanes")


def test_values_windows(pa):
    rng = np.random.default_rng(10)
    pairs = []
    for w0 in WINDOWS:
        for w1 in WINDOWS:
            p = []
            for w in (w0, w1):
                nl = 2 * int(rng.integers(2, 17))
                W = nl // 2
                nwb = W + 4
                a, b = _seqs(rng, int(rng.integers(1, 300)), 64 * nwb - int(rng.integers(0, 64)), int(rng.integers(0, 1 << 30)))
                n = int(rng.integers(1, len(a) + 1))
                p.append(make_job(rng, a, b, int(rng.integers(0, len(a) - n + 1)), n, 2, nl, tap=int(rng.integers(-1, nl)), window=w,
                                  update=bool(rng.integers(0, 2)), hin=bool(rng.integers(0, 2))))
            pairs.append(tuple(p))
    # one half with values, the other without
    for w in WINDOWS:
        p = []
        for with_values in (True, False):
            a, b = _seqs(rng, 200, 900, int(rng.integers(0, 1 << 30)))
            p.append(make_job(rng, a, b, 10, 150, 3, 16, tap=5, window=w if with_values else None))
        pairs.append(tuple(p))
    all_paths(pa, pairs, True, "values windows")


def test_update_pattern(pa):
    """hin == hout: the tapped row is written over the top row it was read from; top and tapped deltas differ."""
    rng = np.random.default_rng(11)
    pairs = []
    for n in (1, 31, 33, 64, 200, 256, 300):
        p = []
        for nl in (32, 12):
            a, b = _seqs(rng, n + 20, 32 * nl + 10, int(rng.integers(0, 1 << 30)))
            job = make_job(rng, a, b, 20, n, 0, nl, tap=nl - 1 if n % 2 else 1, update=True, top="minus" if n % 3 else "random")
            p.append(job)
        pairs.append(tuple(p))
    all_paths(pa, pairs, True, "update")
    want = sp.strip(pairs[-1][0], 1, True)
    assert not np.array_equal(want["hout"][20:320], pairs[-1][0]["hout"][20:320])  # the row really changes


# ---- contents -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap_variant", [False, True])
def test_contents(pa, tap_variant):
    rng = np.random.default_rng(12 + tap_variant)
    jobs = []
    for kind in ("random", "identical", "homopolymer", "absent"):
        for _ in range(8):
            nl = 2 * int(rng.integers(1, 17))
            n = int(rng.integers(1, 300))
            if kind == "random":
                a, b = _seqs(rng, n, 32 * nl, int(rng.integers(0, 1 << 30)))
            elif kind == "identical":
                a = rand_seq(max(n, 32 * nl) + 5, seed=int(rng.integers(0, 1 << 30)))
                b = a[:32 * nl]
            elif kind == "homopolymer":
                x, y = rng.choice(list(b"ACGT"), 2, replace=False)
                a, b = bytes([x]) * n, bytes([y]) * (32 * nl)
            else:  # the first column's base is absent from the first lanes (as test_batch_shapes_low_complexity_first_column)
                a = rand_seq(n, seed=int(rng.integers(0, 1 << 30)))
                others = [c for c in b"ACGT" if c != a[0]]
                head = bytes(others[k] for k in rng.integers(0, 3, 32 * min(nl, 4)))
                b = head + rand_seq(32 * nl - len(head) + int(rng.integers(0, 64)), seed=int(rng.integers(0, 1 << 30)))
            tap = int(rng.integers(-1, nl)) if tap_variant else -1
            jobs.append(make_job(rng, a, b, 0, n, 0, nl, tap=tap, top=("plus", "random")[len(jobs) % 2], left=("plus", "random")[len(jobs) // 2 % 2]))
    all_paths(pa, list(zip(jobs[0::2], jobs[1::2])), tap_variant, "contents")


# ---- random fuzz ----------------------------------------------------------------------------------------------------------------
def _random_job(rng, tap_variant):
    nl = 2 * int(rng.integers(1, 17))
    W = nl // 2
    la = int(rng.integers(1, 400))
    n = int(rng.integers(1, la + 1))
    col0 = int(rng.integers(0, la - n + 1))
    if rng.random() < 0.2:
        la = col0 + n
    nwb = W + int(rng.integers(0, 4))
    lb = 64 * nwb - int(rng.integers(0, 64))
    a, b = _seqs(rng, la, lb, int(rng.integers(0, 1 << 30)))
    if rng.random() < 0.25:  # long diagonal runs
        b = (a * (1 + lb // max(1, la)))[:lb]
    word0 = int(rng.integers(0, nwb - W + 1))
    kinds = ["random", "random", "plus", "minus", "zero"]
    opts = dict(top=kinds[rng.integers(0, 5)], left=kinds[rng.integers(0, 5)], hin=bool(rng.integers(0, 2)))
    if tap_variant:
        opts.update(tap=int(rng.integers(-1, nl)), update=rng.random() < 0.3)
        if rng.random() < 0.4:
            opts["window"] = WINDOWS[rng.integers(0, len(WINDOWS))]
        if opts["update"]:
            opts["hin"] = False
    return make_job(rng, a, b, col0, n, word0, nl, **opts)


@pytest.mark.parametrize("tap_variant", [False, True])
def test_fuzz(pa, tap_variant):
    rng = np.random.default_rng(2024 + tap_variant)
    pairs = [(_random_job(rng, tap_variant), _random_job(rng, tap_variant)) for _ in range(1000)]
    all_paths(pa, pairs, tap_variant, "fuzz", rdv_every=5)


# ---- the rendezvous -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap_variant", [False, True])
@pytest.mark.parametrize("nwaves", [2, 3, 4])
@pytest.mark.parametrize("patience", [0, BIG_PATIENCE])
def test_rdv(pa, tap_variant, nwaves, patience):
    rng = np.random.default_rng(100 * nwaves + tap_variant + (patience > 0))
    groups = 24
    jobs = [_random_job(rng, tap_variant) for _ in range(groups * nwaves)]
    wants = [sp.strip(j, 1, tap_variant) for j in jobs]
    for took, served, alone, _ in run(pa, pa.capi.STRIP_RDV, int(tap_variant), jobs, wants, "rdv", nwaves=nwaves, patience=patience):
        assert took == served and took + served + alone == len(jobs), (took, served, alone)
        if patience and nwaves == 2:
            assert took == groups


# ---- rejected arguments ---------------------------------------------------------------------------------------------------------
def test_rejected_arguments(pa):
    rng = np.random.default_rng(13)
    a, b = _seqs(rng, 100, 300, 5)  # 5 profile words

    def job(tap=-1, window=None, **shape):
        j = make_job(rng, a, b, 0, 50, 0, 4, tap=tap, window=window)
        j.update(shape)
        return j

    good = job()
    cases = [
        (1, 0, [job(n=0)]), (1, 0, [job(col0=60, n=41)]), (1, 0, [job(col0=-1)]),
        (1, 0, [job(word0=3, nlanes=6)]), (1, 2, [job(word0=0, nlanes=12)]), (1, 0, [job(word0=-1)]),
        (1, 0, [job(nlanes=3)]), (1, 0, [job(nlanes=0)]), (0, 0, [job(nlanes=34), good]), (1, 0, [job(nlanes=34)]), (1, 2, [job(nlanes=66)]),
        (1, 1, [job(tap=4)]), (1, 2, [job(tap=4)]), (1, 3, [job(nlanes=8, tap=4)]), (0, 1, [job(tap=4), good]), (1, 0, [job(tap=1)]),
        (0, 0, [job(tap=1), good]), (0, 0, [job(window="contains"), good]), (1, 0, [job(window="contains")]),
        (0, 0, [good]), (1, 4, [good]), (2, 0, [good, good, good]),
    ]
    for mode, variant, jobs in cases:
        with pytest.raises(pa.PaError):
            pa.capi.strip_probe(mode, variant, jobs, nwaves=2)
    with pytest.raises(pa.PaError):
        pa.capi.strip_probe(2, 0, [good] * 5, nwaves=5)
    with pytest.raises(pa.PaError):
        pa.capi.strip_probe(1, 0, [dict(job(), a=b"ACGN" * 25)])
    # and the good job is fine on every path
    run(pa, 1, 0, [good], [sp.strip(good, 1, False)], "good")
    run(pa, 0, 0, [good, good], [sp.strip(good, 1, False)] * 2, "good")
