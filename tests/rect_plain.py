"""A plain model of the rectangle operator (`pa_bp_profile_build`, `pa_bp_compute`, `pa_bp_fill`) and of the device-resident
handle (`pa_bp_ctx_*`), written from the definition on top of `strip_plain.rect_dp`: integers and numpy, one cell at a time in
meaning, no bit vectors, nothing from `oracle/` or `csrc/`.

A rectangle covers columns `a[i0:i1]` and rows `64 w0 .. 64 w1` of `b`.  The rows are read back from `b`'s profile words, so
rows past `|b|` in the last word are the (0, 0) planes and match `T`: that is what the operator is defined over.

* Top row: `D[0][c + 1] = D[0][c] + top[c]`; left column: `D[r + 1][0] = D[r][0] + left[r]`; deltas in {-1, 0, +1}.
* Cell step: `D[r + 1][c + 1] = min(D[r][c] + [row r !~ column c], D[r][c + 1] + 1, D[r + 1][c] + 1)`.
* `rect` -> `(sum, right, bottom)`: `sum = D[H][n] - D[H][0]`, the right column's and the bottom row's deltas.
* `rect_columns` -> the same plus `D[r + 1][c + 1] - D[r][c + 1]` for every column `c`: the `values` of `fill`.
* No rows (`w0 == w1`): the bottom row is the top row.  No columns: the right column is the left one and the sum is 0.

`HandleModel` is `pa_bp_ctx` as include/pa_bitpacking_hip.h states it (blocks.rs:665-748): a stored row `h` of `|a|` deltas, all
zero at first (blocks.rs:119-123), and per call a mode -- None (top +1, bottom dropped), Input (top from `h`, bottom
dropped), Update (top from `h`, bottom stored back), Output (top +1, bottom stored).  With an empty word range that makes
None return `n`, Output store +1 and return `n`, Input and Update return the stored row's sum.  `fill` (blocks.rs:627-648) has a
+1 top row and never touches `h`.

Worked example: `a = CACG`, `b = AG`, columns 1 .. 4 (`ACG`), word 0, top and left all +1.  Rows 0 and 1 are `A` and `G`, rows
2 .. 63 are padding and match `T`, which no column is: below row 2 every cell is the cell above plus one.

    D =  0 1 2 3        row 1 (A): A matches column 0, so D[1][1] = D[0][0] = 0
         1 0 1 2        row 2 (G): G matches column 2, so D[2][3] = D[1][2] = 1
         2 1 1 1        row 3 (padding): D[3][.] = 3 2 2 2, and so on down to row 64
         3 2 2 2

so `sum = D[64][3] - D[64][0] = -1`, the bottom row's deltas are `(-1, 0, 0)`, the right column's `(-1, -1, +1, +1, ..)`, and the
columns `rect_columns` returns start `(-1, +1, +1, ..)`, `(-1, 0, +1, ..)`, `(-1, -1, +1, ..)`.
"""
import numpy as np

from tests.strip_plain import ONE, codes, profile_words, rect_dp, row_codes, v_deltas, v_words

H_NONE, H_INPUT, H_UPDATE, H_OUTPUT = 0, 1, 2, 3
MODE_NAMES = {H_NONE: "None", H_INPUT: "Input", H_UPDATE: "Update", H_OUTPUT: "Output"}


def a_bits(a: bytes) -> np.ndarray:
    """(|a|, 2) uint64: the exploded code bits of `a`, (-(r & 1), -(r >> 1)) with A0 C1 G2 T3 (profile.rs:116-125)."""
    r = codes(a)
    out = np.zeros((len(a), 2), np.uint64)
    out[:, 0] = np.where(r & 1, ONE, np.uint64(0))
    out[:, 1] = np.where(r >> 1, ONE, np.uint64(0))
    return out


def h_words(d) -> np.ndarray:
    """Horizontal deltas -> (n, 2) uint64 H = (p, m), each 0 or 1."""
    d = np.asarray(d, np.int64)
    out = np.zeros((len(d), 2), np.uint64)
    out[:, 0] = d == 1
    out[:, 1] = d == -1
    return out


def h_word_deltas(hw) -> np.ndarray:
    hw = np.asarray(hw, np.uint64).reshape(-1, 2)
    return hw[:, 0].astype(np.int64) - hw[:, 1].astype(np.int64)


def rand_v(rng, w: int) -> np.ndarray:
    """(w, 2) uint64 V words of `64 w` random deltas in {-1, 0, +1}."""
    return v_words(rng.integers(-1, 2, 64 * w))


def _rect(col_codes, prof, w0, w1, top, left):
    s, right, bottom, _ = rect_dp(col_codes, row_codes(prof, w0, 2 * (w1 - w0)), top, left)
    return s, right, bottom


def _rect_columns(col_codes, prof, w0, w1, top, left):
    """One column at a time: each column is a rectangle of its own whose left edge is the column before it."""
    n, rc = len(col_codes), row_codes(prof, w0, 2 * (w1 - w0))
    cols = np.zeros((n, 64 * (w1 - w0)), np.int64)
    bottom = np.zeros(n, np.int64)
    cur = np.asarray(left, np.int64)
    for c in range(n):
        _, cur, bot, _ = rect_dp(col_codes[c : c + 1], rc, top[c : c + 1], cur)
        cols[c], bottom[c] = cur, bot[0]
    return int(bottom.sum()), cur, bottom, cols


def rect(a: bytes, b: bytes, i0: int, i1: int, w0: int, w1: int, top, left):
    """-> (sum of the bottom deltas, right column deltas [64 (w1 - w0)], bottom row deltas [i1 - i0])."""
    return _rect(codes(a)[i0:i1], profile_words(b), w0, w1, np.asarray(top, np.int64), np.asarray(left, np.int64))


def rect_columns(a: bytes, b: bytes, i0: int, i1: int, w0: int, w1: int, top, left):
    """-> rect(..) + (the vertical deltas after every column, [i1 - i0, 64 (w1 - w0)])."""
    return _rect_columns(codes(a)[i0:i1], profile_words(b), w0, w1, np.asarray(top, np.int64), np.asarray(left, np.int64))


def values_words(cols: np.ndarray) -> np.ndarray:
    """The columns of rect_columns -> `values` as fill lays them out: uint64 [n, w, 2]."""
    n, rows = cols.shape
    return v_words(cols.reshape(-1)).reshape(n, rows // 64, 2)


class HandleModel:
    """pa_bp_ctx: `a`, `b` and the stored row of horizontal deltas.  compute / fill return the new v words."""

    def __init__(self, a: bytes, b: bytes):
        self.a, self.b = a, b
        self.words = (len(b) + 63) // 64
        self._codes, self._prof = codes(a), profile_words(b)
        self.h = np.zeros(len(a), np.int64)  # blocks.rs:119-123: H::zero(), not +1

    def compute(self, i0: int, i1: int, w0: int, w1: int, v, mode: int):
        """-> (sum, v words [w1 - w0, 2])."""
        assert 0 <= i0 <= i1 <= len(self.a) and 0 <= w0 <= w1 <= self.words and mode in MODE_NAMES
        top = self.h[i0:i1].copy() if mode in (H_INPUT, H_UPDATE) else np.ones(i1 - i0, np.int64)
        s, right, bottom = _rect(self._codes[i0:i1], self._prof, w0, w1, top, v_deltas(v)[: 64 * (w1 - w0)])
        if mode in (H_UPDATE, H_OUTPUT):
            self.h[i0:i1] = bottom
        return s, v_words(right)

    def fill(self, i0: int, i1: int, w0: int, w1: int, v):
        """-> (values uint64 [i1 - i0, w1 - w0, 2], h_bottom int64 [i1 - i0], v words [w1 - w0, 2])."""
        assert 0 <= i0 <= i1 <= len(self.a) and 0 <= w0 <= w1 <= self.words
        top = np.ones(i1 - i0, np.int64)
        _, right, bottom, cols = _rect_columns(self._codes[i0:i1], self._prof, w0, w1, top, v_deltas(v)[: 64 * (w1 - w0)])
        return values_words(cols), bottom, v_words(right)
