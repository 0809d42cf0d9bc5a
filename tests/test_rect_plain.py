"""The plain rectangle model of tests/rect_plain.py against a literal cell loop, its worked example and the CPU oracle's
operators, so that the GPU operator tests (test_gpu_operator_edges.py) rest on a reference that was checked on its own."""
import numpy as np
import pytest

import oracle
from tests import rect_plain as rp
from tests import strip_plain as sp
from tests.util_seq import rand_seq


def _cells(cols, rows, top, left):
    """The definition, one cell at a time -> the whole matrix D[r][c]."""
    D = np.zeros((len(rows) + 1, len(cols) + 1), np.int64)
    D[0, 1:], D[1:, 0] = np.cumsum(top), np.cumsum(left)
    for r in range(len(rows)):
        for c in range(len(cols)):
            D[r + 1, c + 1] = min(D[r, c] + (rows[r] != cols[c]), D[r, c + 1] + 1, D[r + 1, c] + 1)
    return D


def _oracle_hv(top, left):
    h = np.zeros(len(top), oracle.H_DTYPE)
    h["p"], h["m"] = (np.asarray(top) == 1), (np.asarray(top) == -1)
    vw = sp.v_words(left)
    v = np.zeros(len(vw), oracle.V_DTYPE)
    v["p"], v["m"] = vw[:, 0], vw[:, 1]
    return h, v


def _v_of(v) -> np.ndarray:
    return np.stack([v["p"], v["m"]], axis=-1)


def test_worked_example():
    top, left = np.ones(3, np.int64), np.ones(64, np.int64)
    s, right, bottom = rp.rect(b"CACG", b"AG", 1, 4, 0, 1, top, left)
    assert s == -1 and bottom.tolist() == [-1, 0, 0]
    assert right.tolist() == [-1, -1] + [1] * 62
    s2, right2, bottom2, cols = rp.rect_columns(b"CACG", b"AG", 1, 4, 0, 1, top, left)
    assert (s2, right2.tolist(), bottom2.tolist()) == (s, right.tolist(), bottom.tolist())
    assert cols[:, :3].tolist() == [[-1, 1, 1], [-1, 0, 1], [-1, -1, 1]] and (cols[:, 3:] == 1).all()
    assert rp.a_bits(b"ACGT").tolist() == [[0, 0], [int(sp.ONE), 0], [0, int(sp.ONE)], [int(sp.ONE), int(sp.ONE)]]
    m = rp.HandleModel(b"CACG", b"AG")
    assert m.compute(1, 4, 0, 1, sp.v_words(left), rp.H_OUTPUT)[0] == -1 and m.h.tolist() == [0, -1, 0, 0]


@pytest.mark.parametrize("seed", range(48))
def test_rect_is_the_cell_loop(seed):
    rng = np.random.default_rng(seed)
    a, b = rand_seq(int(rng.integers(1, 40)), seed=100 + seed), rand_seq(int(rng.integers(1, 260)), seed=200 + seed)
    if seed % 3 == 0:  # a shared stretch: long diagonal runs
        b = (a * 8)[: len(b)]
    W = (len(b) + 63) // 64
    w0 = int(rng.integers(0, W)) if seed % 2 else 0
    w1 = int(rng.integers(w0 + 1, W + 1))
    i0 = int(rng.integers(1, len(a))) if len(a) > 1 else 0
    i1 = int(rng.integers(i0 + 1, len(a) + 1))
    top, left = rng.integers(-1, 2, i1 - i0), rng.integers(-1, 2, 64 * (w1 - w0))
    if seed % 5 == 0:
        top[:], left[:] = 1, 1
    rows = np.full(64 * W, 3, np.int64)  # padding rows match T
    rows[: len(b)] = sp.codes(b)
    D = _cells(sp.codes(a)[i0:i1], rows[64 * w0 : 64 * w1], top, left)
    s, right, bottom = rp.rect(a, b, i0, i1, w0, w1, top, left)
    assert s == D[-1, -1] - D[-1, 0]
    assert right.tolist() == np.diff(D[:, -1]).tolist() and bottom.tolist() == np.diff(D[-1, :]).tolist()
    s2, right2, bottom2, cols = rp.rect_columns(a, b, i0, i1, w0, w1, top, left)
    assert (s2, right2.tolist(), bottom2.tolist()) == (s, right.tolist(), bottom.tolist())
    assert cols.tolist() == np.diff(D[:, 1:], axis=0).T.tolist()


def test_rect_without_rows_or_columns():
    top, left = np.array([1, -1, 0, -1]), np.arange(128) % 3 - 1
    s, right, bottom = rp.rect(b"ACGT", b"A" * 100, 0, 4, 1, 1, top, [])
    assert s == -1 and len(right) == 0 and bottom.tolist() == top.tolist()
    s, right, bottom = rp.rect(b"ACGT", b"A" * 100, 2, 2, 0, 2, [], left)
    assert s == 0 and right.tolist() == left.tolist() and len(bottom) == 0
    s, right, bottom, cols = rp.rect_columns(b"ACGT", b"A" * 100, 0, 4, 2, 2, top, [])
    assert s == -1 and bottom.tolist() == top.tolist() and cols.shape == (4, 0) and rp.values_words(cols).shape == (4, 0, 2)


# (columns, words): the word counts straddle 16 / 17, 32 / 33 and 64 / 65
ORACLE_SHAPES = [(1, 1), (5, 15), (33, 16), (40, 17), (17, 31), (64, 32), (31, 33), (20, 63), (16, 64), (9, 65)]


@pytest.mark.parametrize("n,w", ORACLE_SHAPES)
@pytest.mark.parametrize("ragged", [False, True])
def test_rect_against_oracle(n, w, ragged):
    rng = np.random.default_rng(n * 100 + w)
    i0, w0 = int(rng.integers(1, 40)), int(rng.integers(1, 5))
    a = rand_seq(i0 + n + 3, seed=n)
    b = rand_seq(64 * (w0 + w) - (int(rng.integers(1, 64)) if ragged else 0), seed=w + 1)
    top, left = rng.integers(-1, 2, n), rng.integers(-1, 2, 64 * w)
    oa, ob = oracle.bitprofile_build(a, b)
    assert sp.profile_words(b).tolist() == np.stack([ob["b0"], ob["b1"]], axis=1).tolist()
    assert rp.a_bits(a).tolist() == np.stack([oa["b0"], oa["b1"]], axis=1).tolist()
    oa, ob = np.ascontiguousarray(oa[i0 : i0 + n]), np.ascontiguousarray(ob[w0 : w0 + w])
    h, v = _oracle_hv(top, left)
    want = oracle.simd_compute(oa, ob, h, v, True)
    s, right, bottom = rp.rect(a, b, i0, i0 + n, w0, w0 + w, top, left)
    assert s == want
    assert sp.v_words(right).tolist() == _v_of(v).tolist()
    assert rp.h_words(bottom).tolist() == _v_of(h).tolist()
    h, v = _oracle_hv(top, left)
    want, values = oracle.scalar_fill(oa, ob, h, v)
    s, right, bottom, cols = rp.rect_columns(a, b, i0, i0 + n, w0, w0 + w, top, left)
    assert s == want
    assert sp.v_words(right).tolist() == _v_of(v).tolist() and rp.h_words(bottom).tolist() == _v_of(h).tolist()
    assert rp.values_words(cols).tolist() == _v_of(values).tolist()


class _OracleHandle:
    """The same calls played by hand on oracle.simd_compute / scalar_fill with an explicit h array (blocks.rs:729-747)."""

    def __init__(self, a, b):
        self.oa, self.ob = oracle.bitprofile_build(a, b)
        self.h = np.zeros(len(a), oracle.H_DTYPE)

    def compute(self, i0, i1, w0, w1, vw, mode):
        v = np.zeros(w1 - w0, oracle.V_DTYPE)
        v["p"], v["m"] = vw[:, 0], vw[:, 1]
        oa, ob = np.ascontiguousarray(self.oa[i0:i1]), np.ascontiguousarray(self.ob[w0:w1])
        if mode == rp.H_NONE:
            s = oracle.simd_compute(oa, ob, oracle.ones_h(i1 - i0), v, True)
        elif mode == rp.H_INPUT:
            s = oracle.simd_compute(oa, ob, self.h[i0:i1].copy(), v, True)
        else:
            h = oracle.ones_h(i1 - i0) if mode == rp.H_OUTPUT else self.h[i0:i1].copy()
            s = oracle.simd_compute(oa, ob, h, v, True)
            self.h[i0:i1] = h
        return s, _v_of(v)


def _script(W):
    O, I, U, N = rp.H_OUTPUT, rp.H_INPUT, rp.H_UPDATE, rp.H_NONE
    return [
        (I, 0, 50, 0, 3),       # Input over the never-written row: zeros, not +1
        (N, 3, 77, 1, W),       # None ...
        (I, 3, 77, 0, 2),       # ... then Input: None stored nothing
        (O, 10, 60, 0, 2),
        (I, 10, 60, 2, W),
        (U, 10, 60, 2, 5),      # Update twice over the same row
        (U, 10, 60, 5, W),
        (I, 5, 70, 0, 1),       # stored, and never-written columns on both sides
        (O, 20, 40, 3, 3),      # Output on an empty range: stores +1, returns n
        (I, 15, 45, 1, 4),
        (U, 0, 90, 4, 4),       # Update on an empty range: the row's sum, row kept
        (I, 0, 90, W, W),
        (N, 33, 90, 2, 2),      # None on an empty range: n
        (U, 17, 17, 0, W),      # no columns
        (I, 0, 90, 0, W),
    ]


def test_handle_model_against_oracle_script():
    rng = np.random.default_rng(5)
    a, b = rand_seq(90, seed=11), rand_seq(64 * 7 - 13, seed=12)
    W = 7
    model, byhand = rp.HandleModel(a, b), _OracleHandle(a, b)
    for k, (mode, i0, i1, w0, w1) in enumerate(_script(W)):
        v = rp.rand_v(rng, w1 - w0)
        s, v2 = model.compute(i0, i1, w0, w1, v, mode)
        if i1 > i0:
            want, want_v = byhand.compute(i0, i1, w0, w1, v, mode)
        else:
            want, want_v = 0, v
        assert s == want and v2.tolist() == want_v.tolist(), (k, mode, i0, i1, w0, w1)
        assert rp.h_words(model.h).tolist() == _v_of(byhand.h).tolist(), k
        assert v.tolist() != v2.tolist() or w1 == w0 or i1 == i0  # the input is not mutated into the output


def test_handle_model_empty_word_ranges():
    """None returns n, Output stores +1 and returns n, Input and Update return the stored row's sum (blocks.rs:729-747 with
    no rows: the bottom row is the top row)."""
    a, b = rand_seq(40, seed=1), rand_seq(200, seed=2)
    m = rp.HandleModel(a, b)
    e = np.zeros((0, 2), np.uint64)
    assert m.compute(0, 40, 2, 2, e, rp.H_INPUT)[0] == 0 and not m.h.any()
    assert m.compute(5, 30, 1, 1, e, rp.H_NONE)[0] == 25 and not m.h.any()
    assert m.compute(5, 30, 1, 1, e, rp.H_OUTPUT)[0] == 25 and m.h.tolist() == [0] * 5 + [1] * 25 + [0] * 10
    assert m.compute(0, 40, 0, 0, e, rp.H_INPUT)[0] == 25 and m.compute(20, 40, 4, 4, e, rp.H_UPDATE)[0] == 10
    assert m.h.tolist() == [0] * 5 + [1] * 25 + [0] * 10


def test_handle_model_fill_against_oracle():
    rng = np.random.default_rng(9)
    a, b = rand_seq(70, seed=21), rand_seq(64 * 5 - 7, seed=22)
    m = rp.HandleModel(a, b)
    m.compute(0, 70, 0, 2, rp.rand_v(rng, 2), rp.H_OUTPUT)
    before = m.h.copy()
    oa, ob = oracle.bitprofile_build(a, b)
    for i0, i1, w0, w1 in [(3, 40, 1, 5), (17, 18, 0, 1), (0, 70, 2, 4), (33, 65, 4, 5)]:
        vw = rp.rand_v(rng, w1 - w0)
        h, v = _oracle_hv(np.ones(i1 - i0, np.int64), sp.v_deltas(vw))
        want, values = oracle.scalar_fill(np.ascontiguousarray(oa[i0:i1]), np.ascontiguousarray(ob[w0:w1]), h, v)
        got_values, hb, v2 = m.fill(i0, i1, w0, w1, vw)
        assert got_values.tolist() == _v_of(values).tolist() and v2.tolist() == _v_of(v).tolist()
        assert rp.h_words(hb).tolist() == _v_of(h).tolist() and int(hb.sum()) == want
        assert m.h.tolist() == before.tolist()  # fill leaves the stored row alone
    values, hb, v2 = m.fill(4, 9, 3, 3, np.zeros((0, 2), np.uint64))
    assert values.shape == (5, 0, 2) and hb.tolist() == [1] * 5 and v2.shape == (0, 2)
