"""Local alignment over the double-affine batch (pa_affine4_batch_run_local / _align_local, csrc/affine4_local_kernel.hpp) against the
plain DP of tests/affine4_local_plain.py: score, four endpoints and exact CIGAR of every pair, plus an independent pricing of the CIGAR,
at the kernel's shape edges (segment widths, strip counts), with planted best cells and ties, a gap that only the second piece affords
across lane and strip boundaries, neighbours in memory, chunks and the score bound."""
import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, AffineCost
from tests import affine4_local_plain as lp4
from tests.test_gpu_affine4 import MODELS, mutate, rand_seq

pytestmark = pytest.mark.gpu

R = pa.capi.AFFINE4_ROWS_PER_LANE
CM = MODELS["double_affine"]  # double_affine(4, 6, 2, 24, 1)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    pa.require_gpu()


def check(pairs, cm, match, results, ends=None):
    assert len(results) == len(pairs)
    for p, ((x, y), got) in enumerate(zip(pairs, results)):
        want = lp4.local_sw4(x, y, cm, match)
        assert got == want, (p, len(x), len(y))
        score, cigar, a0, a1, b0, b1 = got
        assert lp4.local_verify4(cigar, x, y, a0, b0, cm, match) == (score, a1, b1)
    if ends is not None:
        scores, e = ends
        assert scores.tolist() == [r[0] for r in results]
        assert e.dtype == np.int64 and e.shape == (len(pairs), 2)
        assert e.tolist() == [[r[3], r[5]] for r in results]


def traced(pairs, cm, match):
    b = Affine4Batch(pairs, cm, trace=True)
    try:
        res = b.align_sw(match)
        ends = b.run_sw(match)
    finally:
        b.close()
    return res, ends


EDGE_M = [0, 1, R - 1, R, R + 1, 2 * R + 1, 32 * R, 32 * R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 128 * R, 128 * R + 1]
EDGE_N = [0, 1, 40, 130]


def edge_pairs(seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for k, m in enumerate(EDGE_M):
        y = rand_seq(rng, m)
        for q, n in enumerate(EDGE_N):
            if (k + q) % 2:  # a mutated copy of a window of b
                lo = int(rng.integers(0, max(m - n, 0) + 1))
                x = mutate(rng, y[lo:lo + n], 0.15)[:n]
                x += rand_seq(rng, n - len(x))
            else:
                x = rand_seq(rng, n)
            pairs.append((x, y))
    return pairs


@pytest.mark.parametrize("match", (1, 2, 1000))
@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_model_at_the_shape_edges(name, match):
    pairs = edge_pairs(len(name) + match)
    res, ends = traced(pairs, MODELS[name], match)
    check(pairs, MODELS[name], match, res, ends)


def planted(rng, n, m, spots):
    """a over GT and b over AC, with nothing in common but the words of `spots`: (word, i_end, j_end), over alphabets of their own."""
    a, b = bytearray(rand_seq(rng, n, b"GT")), bytearray(rand_seq(rng, m, b"AC"))
    for word, i_end, j_end in spots:
        a[i_end - len(word):i_end] = word
        b[j_end - len(word):j_end] = word
    return bytes(a), bytes(b)


WORD, WORD2 = b"NRYKMSWBDHVU", b"nrykmswbdhvu"  # no byte twice, none of ACGT, nothing shared
L = len(WORD)


@pytest.mark.parametrize("match", (1, 7))
def test_planted_best_cell(match):
    rng = np.random.default_rng(5)
    pairs, want = [], []
    for m in (64 * R + 40, 130 * R):
        for n in (L, 150):
            for j in (R, R + 1, 64 * R, 64 * R + 1, m):
                for i in (L, n):
                    pairs.append(planted(rng, n, m, [(WORD, i, j)]))
                    want.append((L * match, f"{L}=", i - L, i, j - L, j))
    res, ends = traced(pairs, CM, match)
    assert res == want
    check(pairs, CM, match, res, ends)


def test_ties():
    rng = np.random.default_rng(6)
    m, n = 70 * R, 90  # two strips
    cases = (
        ([(WORD, 50, 2 * R), (WORD, 50, 9 * R + 3)], (50, 2 * R)),            # the same i, two j in different lanes: the lower j
        ([(WORD, 50, 3 * R), (WORD, 50, 66 * R)], (50, 3 * R)),               # the same i, two j in different strips
        ([(WORD, 30, 65 * R + 5), (WORD2, 70, 4 * R)], (30, 65 * R + 5)),     # the lower i in strip 1 against the higher i in strip 0
    )
    pairs = [planted(rng, n, m, spots) for spots, _ in cases]
    want = [(2 * L, f"{L}=", i - L, i, j - L, j) for _, (i, j) in cases]
    res, ends = traced(pairs, CM, 2)
    assert res == want
    check(pairs, CM, 2, res, ends)


W1 = bytes(range(0x80, 0x80 + 50))  # two 50-byte words over bytes that occur nowhere else (none of ACGT)
W2 = bytes(range(0xC0, 0xC0 + 50))
assert not set(W1 + W2) & set(b"ACGT") and len(set(W1 + W2)) == 100


def gap_pair(rng, lo, long_len, short_len, in_b):
    """The words next to each other in the short sequence (over GT), and 60 bytes apart in the long one (over AC), where the 60 bytes
    are [lo, lo + 60).  in_b: the long one is b (an insert), else a (a delete).  -> (pair, expected result)"""
    long_, short = bytearray(rand_seq(rng, long_len, b"AC")), bytearray(rand_seq(rng, short_len, b"GT"))
    long_[lo - 50:lo] = W1
    long_[lo + 60:lo + 110] = W2
    s0 = 11
    short[s0:s0 + 100] = W1 + W2
    long_, short = bytes(long_), bytes(short)
    if in_b:
        return (short, long_), (s0, s0 + 100, lo - 50, lo + 110)
    return (long_, short), (lo - 50, lo + 110, s0, s0 + 100)


def test_a_gap_only_the_second_piece_affords():
    # 60 extra bytes between two 50-byte words.  Under double_affine(4, 6, 2, 24, 1) and match = 2 the second piece pays 24 + 60 = 84
    # of the words' 200 and joins them (116); the first piece alone would pay 6 + 120 = 126 and leave 74, less than one word's 100.
    # The insert's rows cross lane boundaries (rows 5 R - 20 .. 5 R + 40: with R = 16 the word before it does not fit above row
    # R - 20), in a second pair the strip boundary (64 R - 20 .. 64 R + 40); the delete's columns run inside the lanes that own the rows.
    rng = np.random.default_rng(13)
    cases = [gap_pair(rng, 5 * R - 20, 12 * R + 3, 130, True), gap_pair(rng, 64 * R - 20, 70 * R, 130, True),
             gap_pair(rng, 75, 300, 64 * R + 30, False)]
    pairs = [p for p, _ in cases]
    want = [(116, "50=60I50=" if k < 2 else "50=60D50=", a0, a1, b0, b1) for k, (_, (a0, a1, b0, b1)) in enumerate(cases)]
    res, ends = traced(pairs, CM, 2)
    assert res == want
    check(pairs, CM, 2, res, ends)
    # with two equal pieces of (6, 2) the words are not joined: the first word alone
    res, ends = traced(pairs, AffineCost.double_affine(4, 6, 2, 6, 2), 2)
    assert res == [(100, "50=", w[2], w[2] + 50, w[4], w[4] + 50) for w in want]
    check(pairs, AffineCost.double_affine(4, 6, 2, 6, 2), 2, res, ends)


def test_neighbours_in_memory():
    # One wavefront of 64 pairs with |b| = 10 and |a| = 0 .. 63 (nmax above most |a|).  The batch uploads a0 b0 a1 b1 ..; here that is one
    # run of a periodic text, so the bytes after each a and after each b continue its best match, and a read past |a| or |b| would raise
    # the score.
    rng = np.random.default_rng(7)
    text = rand_seq(rng, 7) * 400
    pairs, pos = [], 0
    for n in range(64):
        pairs.append((text[pos:pos + n], text[pos + n:pos + n + 10]))
        pos += n + 10
    res, ends = traced(pairs, CM, 2)
    check(pairs, CM, 2, res, ends)
    assert max(r[0] for r in res) == 20 and min(r[0] for r in res) == 0


def test_nothing_in_common():
    rng = np.random.default_rng(8)
    pairs = [(rand_seq(rng, n, b"GT"), rand_seq(rng, m, b"AC")) for n, m in ((40, 30), (5, 65 * R), (130, R + 1))]
    pairs += [(b"", rand_seq(rng, 20)), (rand_seq(rng, 20), b""), (b"", b"")]
    res, ends = traced(pairs, CM, 3)
    assert res == [(0, "", 0, 0, 0, 0)] * len(pairs)
    check(pairs, CM, 3, res, ends)


def random_pairs(seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(2000):
        n, m = int(rng.integers(0, 81)), int(rng.integers(0, 81))
        y = rand_seq(rng, m)
        pairs.append((mutate(rng, y, 0.2)[:n] if k % 3 else rand_seq(rng, n), y))
    for k in range(40):
        lo, hi = ((81, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 2100))[k % 5]  # segments of 16, 32, 64 lanes; two, three strips
        m = int(rng.integers(lo, hi + 1))
        n = int(rng.integers(1, 301))
        y = rand_seq(rng, m)
        lo = int(rng.integers(0, m))
        pairs.append((mutate(rng, y[lo:lo + n], 0.1)[:n], y))
    return [pairs[k] for k in rng.permutation(len(pairs))]


def test_seeded_random():
    pairs = random_pairs(9)
    cm = MODELS["linear_edges"]
    res, ends = traced(pairs, cm, 2)
    check(pairs, cm, 2, res, ends)
    lanes = [max((len(y) + R - 1) // R, 1) for _, y in pairs]
    assert {1 << (k - 1).bit_length() if k <= 64 else 128 for k in lanes} == {1, 2, 4, 8, 16, 32, 64, 128}  # every segment width, and strips
    assert {(len(y) + 64 * R - 1) // (64 * R) for _, y in pairs} >= {1, 2, 3}


def test_chunks(monkeypatch):
    rng = np.random.default_rng(10)
    pairs = []
    for k in range(12):
        y = rand_seq(rng, 300 + 40 * k)
        pairs.append((mutate(rng, y, 0.1)[:700], y))
    b = Affine4Batch(pairs, CM, trace=True)
    try:
        whole = b.align_sw(2)
        assert b.sw_info()["chunks"] == 1
        monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "2")  # a pair's codes are up to 0.7 MiB: at least 3 chunks
        parts = b.align_sw(2)
        info = b.sw_info()
        assert info["chunks"] >= 3 and 0 < info["bytes_max"] <= 2 << 20
        assert parts == whole
        check(pairs, CM, 2, whole)
    finally:
        b.close()
    big = [(rand_seq(rng, 1100), rand_seq(rng, 1100)), (b"ACGT", b"ACGT")]
    monkeypatch.setenv("PA_AFFINE_TRACE_BUDGET_MB", "1")
    b = Affine4Batch(big, CM, trace=True)
    try:
        with pytest.raises(ValueError, match=r"pa_affine4_batch_align_local: pair 0:"):
            b.align_sw(2)
        scores, _ = b.run_sw(2)  # the cost-only call keeps no codes
        assert scores[1] == 8
    finally:
        b.close()


def test_score_bound():
    cm = AffineCost.double_affine(1, 1, 1, 1, 1)  # (the batch's own bound is (|a| + |b| + 1) * max edge < 2^30)
    long = b"A" * 1_073_742
    b = Affine4Batch([(b"ACGT", b"ACGT"), (long, long)], cm)
    try:
        with pytest.raises(ValueError, match=r"pa_affine4_batch_run_local: pair 1:"):  # 1000 * 1 073 742 >= 2^30: nothing is launched
            b.run_sw(1000)
    finally:
        b.close()
    s = rand_seq(np.random.default_rng(11), 2000)
    res, ends = traced([(s, s)], cm, 1000)
    assert res == [(2_000_000, "2000=", 0, 2000, 0, 2000)] and ends[0].tolist() == [2_000_000]


def test_nothing_else_moves():
    rng = np.random.default_rng(12)
    pairs = []
    for m in (5, 40, 200, 70 * R):
        y = rand_seq(rng, m)
        pairs.append((rand_seq(rng, 30) + mutate(rng, y, 0.05) + rand_seq(rng, 30), y))
    big = (1 << 30) - 1

    def others(b):
        b.set_free_ends(False, False)
        out = [b.run().tolist(), b.align()]
        b.set_free_ends(True, True)
        out += [b.run().tolist(), b.ends().tolist(), b.align(), b.ends().tolist()]
        b.set_free_ends(False, False)  # (the diagonal-transition route takes global batches)
        out += [b.align_tiled(), b.run_dt(big).tolist()]
        b.set_chain(True)
        out.append(b.run().tolist())
        b.set_chain(False)
        return out

    b = Affine4Batch(pairs, CM, trace=True)
    try:
        before = others(b)
        b.run()
        ends_before = b.ends().tolist()
        res, ends = b.align_sw(2), b.run_sw(2)
        assert b.ends().tolist() == ends_before  # neither call touches what ends() reports
        check(pairs, CM, 2, res, ends)
        assert others(b) == before
    finally:
        b.close()


def test_align_local_picks_the_batch_by_the_layers():
    rng = np.random.default_rng(14)
    pairs = []
    for m in (0, 30, 200, 65 * R):
        y = rand_seq(rng, m)
        pairs.append((rand_seq(rng, 20) + mutate(rng, y, 0.1) + rand_seq(rng, 20), y))
    b = Affine4Batch(pairs, CM, trace=True)
    try:
        assert pa.align_local(pairs, CM, 2) == b.align_sw(2)
    finally:
        b.close()
    cm2 = AffineCost.affine(4, 6, 2)
    b = AffineBatch(pairs, cm2, trace=True)
    try:
        assert pa.align_local(pairs, cm2, 2) == b.align_local(2)
    finally:
        b.close()
