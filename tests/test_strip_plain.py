"""The plain rectangle DP of tests/strip_plain.py against its worked example and the CPU oracle's kernels, so that the GPU
strip tests (test_gpu_strip_dual.py) rest on a reference that was checked on its own."""
import numpy as np
import pytest

import oracle
from tests import strip_plain as sp
from tests.util_seq import rand_seq


def _deltas(rng, k: int, kind: str) -> np.ndarray:
    if kind == "random":
        return rng.integers(-1, 2, k).astype(np.int64)
    return np.full(k, {"plus": 1, "minus": -1, "zero": 0}[kind], np.int64)


def test_worked_example():
    s, right, bottom, tapped = sp.rect_dp(sp.codes(b"ACG"), sp.codes(b"AG"), [1, 1, 1], [1, 1], tap_row=1)
    assert s == -1
    assert right.tolist() == [-1, -1] and bottom.tolist() == [-1, 0, 0] and tapped.tolist() == [-1, 1, 1]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 100, 128, 129, 1000])
def test_row_codes_are_b(m):
    b = rand_seq(m, seed=m)
    prof = sp.profile_words(b)
    _, pb = oracle.bitprofile_build(b"A", b)
    assert prof[:, 0].tolist() == pb["b0"].tolist() and prof[:, 1].tolist() == pb["b1"].tolist()
    rc = sp.row_codes(prof, 0, 2 * len(prof))
    assert rc[:m].tolist() == sp.codes(b).tolist()
    assert (rc[m:] == 3).all()  # padded rows match T, as the kernels see them
    assert sp.v_deltas(sp.v_words(np.arange(128) % 3 - 1)).tolist() == (np.arange(128) % 3 - 1).tolist()


@pytest.mark.parametrize("seed", range(40))
def test_rect_against_oracle_simd_compute(seed):
    rng = np.random.default_rng(seed)
    a, b = rand_seq(int(rng.integers(1, 400)), seed=1000 + seed), rand_seq(int(rng.integers(1, 1200)), seed=2000 + seed)
    if seed % 4 == 0:  # a shared stretch: long diagonal runs
        b = a[: len(b)] + b[len(a) :]
    nwb = (len(b) + 63) // 64
    n = int(rng.integers(1, len(a) + 1))
    col0 = int(rng.integers(0, len(a) - n + 1))
    W = int(rng.integers(1, nwb + 1))
    word0 = int(rng.integers(0, nwb - W + 1))
    kinds = ["random", "plus", "minus", "zero"]
    top, left = _deltas(rng, n, kinds[seed % 4]), _deltas(rng, 64 * W, kinds[(seed // 4) % 4])
    pa_, pb_ = oracle.bitprofile_build(a, b)
    h = np.zeros(n, oracle.H_DTYPE)
    h["p"], h["m"] = (top == 1), (top == -1)
    vw = sp.v_words(left)
    v = np.zeros(W, oracle.V_DTYPE)
    v["p"], v["m"] = vw[:, 0], vw[:, 1]
    want = oracle.simd_compute(np.ascontiguousarray(pa_[col0 : col0 + n]), np.ascontiguousarray(pb_[word0 : word0 + W]), h, v, True)
    s, right, bottom, _ = sp.rect_dp(sp.codes(a)[col0 : col0 + n], sp.row_codes(sp.profile_words(b), word0, 2 * W), top, left)
    assert s == want
    assert sp.v_words(right)[:, 0].tolist() == v["p"].tolist() and sp.v_words(right)[:, 1].tolist() == v["m"].tolist()
    assert bottom.tolist() == (h["p"].astype(np.int64) - h["m"].astype(np.int64)).tolist()


@pytest.mark.parametrize("seed", range(12))
def test_tapped_row_against_oracle_scalar_fill(seed):
    """A row inside the rectangle, from the columns scalar_fill returns: h[r][c] = h[0][c] + sum over rows < r of (v_{c+1} - v_c)."""
    rng = np.random.default_rng(100 + seed)
    a, b = rand_seq(int(rng.integers(1, 200)), seed=3000 + seed), rand_seq(int(rng.integers(65, 700)), seed=4000 + seed)
    nwb = (len(b) + 63) // 64
    W = int(rng.integers(1, nwb + 1))
    nlanes = 2 * W
    tap = int(rng.integers(0, nlanes - 1))  # rows 32 (tap + 1) < 32 nlanes: a row strictly inside
    r = 32 * (tap + 1)
    top, left = _deltas(rng, len(a), "random"), _deltas(rng, 64 * W, "random")
    pa_, pb_ = oracle.bitprofile_build(a, b)
    h = np.zeros(len(a), oracle.H_DTYPE)
    h["p"], h["m"] = (top == 1), (top == -1)
    vw = sp.v_words(left)
    v = np.zeros(W, oracle.V_DTYPE)
    v["p"], v["m"] = vw[:, 0], vw[:, 1]
    _, values = oracle.scalar_fill(pa_, np.ascontiguousarray(pb_[:W]), h, v)
    cols = [left] + [sp.v_deltas(np.stack([values[c]["p"], values[c]["m"]], axis=1)) for c in range(len(a))]
    want = [int(top[c] + np.sum(cols[c + 1][:r]) - np.sum(cols[c][:r])) for c in range(len(a))]
    _, _, _, tapped = sp.rect_dp(sp.codes(a), sp.row_codes(sp.profile_words(b), 0, nlanes), top, left, tap_row=r)
    assert tapped.tolist() == want


def test_strip_job_windows_and_update():
    """strip(): `values` replaces v inside its window (+1 outside), the Update pattern reads its top row from hout, words and
    bytes outside the strip are kept."""
    rng = np.random.default_rng(7)
    a, b = rand_seq(90, seed=1), rand_seq(300, seed=2)
    v = sp.v_words(rng.integers(-1, 2, 320))
    values = sp.v_words(rng.integers(-1, 2, 320))
    hout = sp.h_bytes(rng.integers(-1, 2, 90))
    job = dict(a=a, b=b, col0=5, n=70, word0=1, nlanes=6, v=v, hout=hout, hin_is_hout=1, tap=3, values=values, fill_word0=2, fill_stride=4)
    got = sp.strip(job)
    left = np.concatenate([np.ones(64, np.int64), sp.v_deltas(values[2:4])])
    s, right, _, tapped = sp.rect_dp(sp.codes(a)[5:75], sp.row_codes(sp.profile_words(b), 1, 6), sp.h_deltas(hout[5:75]), left, tap_row=128)
    assert got["sum"] == s
    assert got["v"][1:4].tolist() == sp.v_words(right).tolist() and got["v"][[0, 4]].tolist() == v[[0, 4]].tolist()
    assert got["hout"][5:75].tolist() == sp.h_bytes(tapped).tolist()
    assert got["hout"][:5].tolist() == hout[:5].tolist() and got["hout"][75:].tolist() == hout[75:].tolist()
