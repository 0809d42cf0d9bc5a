"""The batched semi-global search (`pa.SearchBatch`, pa_search_batch_*): the segment kernel that packs 64 / g queries into one
wavefront, the chained strips of longer patterns, the best-hit reduction and the batched traceback.

Every value is compared with `pa.search` / `pa.search_trace` (one query per call) and, where the shapes allow, with the plain DP of
tests/search_plain.py.  Every batch runs twice.
"""
import math

import numpy as np
import pytest

from tests import search_plain as sp
from tests.util_seq import mutate, rand_seq

pytestmark = pytest.mark.gpu

PLENS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
WILD = b"NnYyRr*"


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


def _pattern(rng, plen: int) -> bytes:
    p = bytearray(b"ACGT"[k] for k in rng.integers(0, 4, plen))
    for k in np.flatnonzero(rng.random(plen) < 0.1):
        p[k] = WILD[rng.integers(0, len(WILD))]
    return bytes(p)


def _plant(rng, text: bytes, pattern: bytes, at: int, rate: float, seed: int) -> bytes:
    """text with a noisy copy of pattern (wildcards resolved to some base) written over it at `at`."""
    core = bytes(b"ACGT"[rng.integers(0, 4)] if c in b"NYR*" else c for c in pattern.upper())
    m = mutate(core, rate, seed) if core else b""
    at = max(0, min(at, len(text)))
    return (text[:at] + m + text[at:])[: len(text)]


def _model_g(plen: int) -> int:
    g = 1
    while 32 * g < plen:
        g *= 2
    return g


def _run_twice(sb):
    c1, i1 = sb.run()
    c2, i2 = sb.run()
    assert np.array_equal(c1, c2) and np.array_equal(i1, i2), "second run differs"
    return c1.copy(), i1.copy()


def _best(out):
    a = np.asarray(out)
    return int(a.min()), int(np.argmin(a))


def test_packing_edges(pa):
    """Rows of every query of one mixed batch equal pa.search and the plain DP: every segment width, the chained strips, texts
    shorter than the padding and at the chunk edges."""
    rng = np.random.default_rng(1)
    patterns = [_pattern(rng, n) for n in PLENS]
    tls = [0, 1, 20, 31, 32, 33, 3000]
    texts = []
    for k, n in enumerate(tls):
        t = rand_seq(n, seed=10 + k)
        if n >= 3000:
            t = _plant(rng, t, patterns[10], 1000, 0.05, 3)
            t = _plant(rng, t, patterns[3], n - 20, 0.0, 4)  # a right-column hit
        texts.append(t.lower() if k % 2 else t)
    queries = [(i, j) for i in range(len(patterns)) for j in range(len(texts))]
    for uc in (0.3, 0.0):
        sb = pa.SearchBatch(patterns, texts, queries, uc)
        costs, idx = _run_twice(sb)
        rows = sb.rows()
        assert all(np.array_equal(a, b) for a, b in zip(sb.rows(), rows))
        for q, (i, j) in enumerate(queries):
            want = pa.search(patterns[i], texts[j], uc)
            assert rows[q].tolist() == want, (len(patterns[i]), len(texts[j]), uc)
            if len(patterns[i]) * len(texts[j]) <= 4097 * 3000:
                assert want == sp.search(patterns[i], texts[j], uc), (len(patterns[i]), len(texts[j]))
            assert (int(costs[q]), int(idx[q])) == _best(want), (len(patterns[i]), len(texts[j]))
        info = sb.info()
        chained = sum(len(texts) for n in PLENS if n > 2048)
        assert info["chained"] == chained and info["packed"] == len(queries) - chained
        sb.close()


def test_best_hit_ties_and_right_column(pa):
    """(best cost, lowest index) against numpy over pa.search: repeated texts give ties, hanging patterns right-column hits."""
    rng = np.random.default_rng(2)
    patterns, texts = [], []
    for k in range(40):
        plen = int(rng.integers(1, 300))
        p = _pattern(rng, plen)
        unit = rand_seq(int(rng.integers(plen + 1, plen + 40)), seed=100 + k)
        unit = _plant(rng, unit, p, 3, 0.0, k)
        t = unit * int(rng.integers(2, 6))
        if k % 3 == 0:  # only the pattern's first half at the end of the text: the best hit is in the right column
            t = rand_seq(500, seed=200 + k) + p[: plen // 2].upper().replace(b"N", b"A").replace(b"Y", b"C").replace(b"R", b"G").replace(b"*", b"T")
        patterns.append(p)
        texts.append(t)
    queries = [(k, k) for k in range(40)] + [(k, (k + 1) % 40) for k in range(40)]
    sb = pa.SearchBatch(patterns, texts, queries, 0.5)
    costs, idx = _run_twice(sb)
    right = 0
    for q, (i, j) in enumerate(queries):
        want = pa.search(patterns[i], texts[j], 0.5)
        assert (int(costs[q]), int(idx[q])) == _best(want), q
        right += int(idx[q]) > len(texts[j])
    assert right > 0


def test_independence(pa):
    """A query gives the same result alone, in reversed, shuffled and duplicated batches, next to texts of very different length."""
    rng = np.random.default_rng(3)
    patterns = [_pattern(rng, int(n)) for n in rng.integers(1, 700, 30)]
    texts = [rand_seq(int(n), seed=300 + k) for k, n in enumerate([5, 40, 100, 900, 5000, 20000])]
    base = [(int(rng.integers(0, 30)), int(rng.integers(0, 6))) for _ in range(60)]
    alone = {}
    for q in base[:12]:
        sb = pa.SearchBatch(patterns, texts, [q], 0.25)
        c, i = _run_twice(sb)
        alone[q] = (int(c[0]), int(i[0]), sb.rows()[0].tolist())
        sb.close()
    perm = list(rng.permutation(len(base)))
    for order in (base, base[::-1], [base[k] for k in perm], base + base):
        sb = pa.SearchBatch(patterns, texts, order, 0.25)
        c, i = _run_twice(sb)
        rows = sb.rows()
        for k, q in enumerate(order):
            if q in alone:
                assert (int(c[k]), int(i[k]), rows[k].tolist()) == alone[q]
        sb.close()


def test_shared_text(pa):
    """300 patterns in one 1 Mbp text (uploaded once) with planted hits: pa.search on a stride of the queries, the plain DP on
    every hit's window."""
    rng = np.random.default_rng(4)
    tlen = 1_000_000
    text = rand_seq(tlen, seed=4)
    patterns = []
    for k in range(300):  # one hit per 3300 bp stretch, so that no two overlap
        plen = int(rng.integers(20, 400))
        p = _pattern(rng, plen)
        text = _plant(rng, text, p, 3300 * k + int(rng.integers(0, 2800)), 0.03, 1000 + k)
        patterns.append(p)
    # unmatched_cost 1: the left column of the whole text equals the all-+1 column of a window, so the plain DP over the window
    # text[end - 2 plen .. end) ends at the same cost (the traceback's first re-fill)
    sb = pa.SearchBatch(patterns, [text], [(k, 0) for k in range(300)], 1.0)
    costs, idx = _run_twice(sb)
    for k in range(0, 300, 30):
        assert (int(costs[k]), int(idx[k])) == _best(pa.search(patterns[k], text, 1.0)), k
    for k in range(300):
        end, plen = int(idx[k]), len(patterns[k])
        assert end <= tlen
        win = text[max(0, end - 2 * plen): end]
        assert sp.search(patterns[k], win, 1.0)[len(win)] == int(costs[k]), k
        assert int(costs[k]) <= math.ceil(0.2 * plen) + 2, (k, int(costs[k]))


def _path(start, cigar):
    i, j = start
    path = [(i, j)]
    for op in sp.cigar_ops(cigar):
        di, dj = sp._STEP[op]
        i, j = i + di, j + dj
        path.append((i, j))
    return path


def _trace_batch(pa, uc):
    rng = np.random.default_rng(5)
    patterns = [_pattern(rng, n) for n in (0, 1, 17, 64, 150, 300, 1025, 2500)]
    texts = [rand_seq(0, seed=1), rand_seq(10, seed=2)]
    for k, p in enumerate(patterns):
        t = rand_seq(3 * len(p) + 50, seed=500 + k)
        t = _plant(rng, t, p, len(t) // 2, 0.08, 600 + k)
        texts.append(t)
    queries = [(i, j) for i in range(len(patterns)) for j in range(len(texts)) if j < 2 or j == i + 2 or (i + j) % 5 == 0]
    sb = pa.SearchBatch(patterns, texts, queries, uc)
    costs, best = _run_twice(sb)
    rows = sb.rows()
    picks = [int(b) for b in best]
    rnd = []
    for q, (i, j) in enumerate(queries):
        n, m = len(patterns[i]), len(texts[j])
        rnd.append(int(rng.integers(0, n + m + 1)) if q % 2 else min(n + m, m + 1 + (q % max(n, 1))))  # every other one in the right column
    for idx in (None, rnd):
        got = sb.trace(idx)
        assert sb.trace(idx) == got
        for q, (i, j) in enumerate(queries):
            k = picks[q] if idx is None else idx[q]
            cigar, path = pa.search_trace(patterns[i], texts[j], uc, k)
            assert got[q] == (cigar, path[0]), (q, len(patterns[i]), len(texts[j]), k)
            sp.check_trace(patterns[i], texts[j], uc, k, rows[q].tolist(), got[q][0], _path(got[q][1], got[q][0]))
    return sb, queries, patterns, texts


def test_trace(pa):
    """CIGAR and start of the best hit and of random indices (right-column ones included) equal pa.search_trace; the plain DP's
    check accepts them."""
    _trace_batch(pa, 0.3)


def test_trace_in_many_chunks(pa, monkeypatch):
    """Device-memory budgets that split the traceback into chunks of one query each (at least 8 chunks) and into chunks of a few
    queries give the same alignments."""
    _, queries, patterns, texts = _trace_batch(pa, 0.0)
    assert len(queries) >= 8
    monkeypatch.setenv("PA_SEARCH_TRACE_BUDGET_MB", "1e-6")  # below any query's re-fill: one query per chunk
    _trace_batch(pa, 0.0)
    per = [min(2 * len(patterns[i]), len(texts[j])) * math.ceil(len(patterns[i]) / 64) * 16 for i, j in queries]
    monkeypatch.setenv("PA_SEARCH_TRACE_BUDGET_MB", str(2 * max(per) / 1048576.0))
    _trace_batch(pa, 0.0)


def test_info_matches_plan_model(pa):
    """waves = sum over g of ceil(queries_g / (64 / g)) + the chained strips; lane use = pattern lanes / launched lanes."""
    rng = np.random.default_rng(6)
    lens = [0, 5, 32, 33, 64, 100, 200, 300, 600, 1000, 2000, 2048, 2049, 3000, 7000]
    patterns = [_pattern(rng, n) for n in lens]
    texts = [rand_seq(n, seed=n) for n in (0, 50, 400, 3000)]
    queries = [(int(rng.integers(0, len(lens))), int(rng.integers(0, 4))) for _ in range(500)]
    sb = pa.SearchBatch(patterns, texts, queries, 0.1)
    per_g = {}
    strips = 0
    for i, j in queries:
        plen = lens[i]
        if plen <= 2048:
            per_g[_model_g(plen)] = per_g.get(_model_g(plen), 0) + 1
        elif len(texts[j]) > 0:
            strips += math.ceil(plen / 64 / 32)
    waves = sum(math.ceil(n / (64 // g)) for g, n in per_g.items()) + strips
    info = sb.info()
    assert info["waves"] == waves
    assert info["packed"] == sum(per_g.values()) and info["chained"] == len(queries) - info["packed"]
    assert info["lane_use"] == pytest.approx(sum(math.ceil(lens[i] / 32) for i, _ in queries) / (64 * waves))
    costs, idx = _run_twice(sb)
    for q in range(0, 500, 37):
        i, j = queries[q]
        assert (int(costs[q]), int(idx[q])) == _best(pa.search(patterns[i], texts[j], 0.1))


def test_no_pack_switch(pa, monkeypatch):
    """PA_SEARCH_BATCH_NO_PACK=1: every query on strips of its own, the same results."""
    rng = np.random.default_rng(7)
    patterns = [_pattern(rng, n) for n in (0, 1, 40, 150, 700, 2100)]
    texts = [rand_seq(n, seed=n) for n in (0, 7, 500, 2000)]
    queries = [(i, j) for i in range(6) for j in range(4)]
    sb = pa.SearchBatch(patterns, texts, queries, 0.5)
    want = _run_twice(sb), sb.rows(), sb.trace()
    monkeypatch.setenv("PA_SEARCH_BATCH_NO_PACK", "1")
    nb = pa.SearchBatch(patterns, texts, queries, 0.5)
    assert nb.info()["packed"] == 0 and nb.info()["chained"] == len(queries)
    got = _run_twice(nb), nb.rows(), nb.trace()
    assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0]))
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    assert got[2] == want[2]


def test_size_100k_reads(pa):
    """100 000 reads of 150 bp in 500 bp windows: best hits against pa.search on a stride."""
    rng = np.random.default_rng(8)
    n = 100_000
    genome = rand_seq(n // 10 * 50 + 1000, seed=8)
    reads, windows = [], []
    for k in range(n):
        at = (k * 50) % (len(genome) - 600)
        win = genome[at: at + 500]
        reads.append(mutate(win[175:325], 0.05, k))
        windows.append(win)
    sb = pa.SearchBatch(reads, windows, [(k, k) for k in range(n)], 0.0)
    per_g = {}
    for r in reads:
        per_g[_model_g(len(r))] = per_g.get(_model_g(len(r)), 0) + 1
    waves = sum(math.ceil(c / (64 // g)) for g, c in per_g.items())
    info = sb.info()
    assert info["waves"] == waves and info["packed"] == n
    assert info["lane_use"] == pytest.approx(sum(math.ceil(len(r) / 32) for r in reads) / (64 * waves))
    costs, idx = _run_twice(sb)
    for k in range(0, n, 997):
        assert (int(costs[k]), int(idx[k])) == _best(pa.search(reads[k], windows[k], 0.0)), k
    assert float(np.mean(costs)) < 15


def test_errors(pa):
    ok_p, ok_t = [b"ACGT", b"ACG"], [b"ACGTACGT", b"TTTT"]
    with pytest.raises(ValueError, match="query 3"):
        pa.SearchBatch(ok_p + [b"ACXT"], ok_t, [(0, 0), (1, 1), (0, 1), (2, 0)], 0.5)
    with pytest.raises(ValueError, match="query 2"):
        pa.SearchBatch(ok_p, ok_t + [b"ACNT"], [(0, 0), (1, 1), (0, 2)], 0.5)
    L = pa.capi.load()
    import ctypes as C

    pp = (C.c_char_p * 2)(*ok_p)
    tp = (C.c_char_p * 2)(*ok_t)
    pl = np.array([4, 3], np.uint64)
    tl = np.array([8, 4], np.uint64)
    for uc in (-0.1, 1.5, float("nan")):
        qp, qt = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        assert not L.pa_search_batch_create(pp, pa.capi._p(pl), 2, tp, pa.capi._p(tl), 2, pa.capi._p(qp), pa.capi._p(qt), 1, C.c_float(uc))
    for qpv, qtv in ((2, 0), (0, 2)):
        qp, qt = np.array([qpv], np.uint32), np.array([qtv], np.uint32)
        assert not L.pa_search_batch_create(pp, pa.capi._p(pl), 2, tp, pa.capi._p(tl), 2, pa.capi._p(qp), pa.capi._p(qt), 1, C.c_float(0.5))
        assert "out of range" in pa.capi.last_error()
    big = np.array([4, (1 << 30) + 1], np.uint64)
    qp, qt = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    assert not L.pa_search_batch_create(pp, pa.capi._p(pl), 2, tp, pa.capi._p(big), 2, pa.capi._p(qp), pa.capi._p(qt), 1, C.c_float(0.5))
    sb = pa.SearchBatch(ok_p, ok_t, [(0, 0), (1, 1)], 0.5)
    with pytest.raises(pa.PaError, match="out of range"):
        sb.trace([0, 8])
    assert [len(r) for r in (sb.trace([12, 7]))] == [2, 2]
    empty = pa.SearchBatch(ok_p, ok_t, [], 0.5)
    c, i = empty.run()
    assert len(c) == 0 and len(i) == 0 and empty.rows() == [] and empty.trace() == [] and empty.info()["waves"] == 0
