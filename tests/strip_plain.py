"""A plain dynamic-programming reference for one strip of the batched A*PA2 band search (`run_strip`, `run_strip_dual`,
`rdv_strip`), written from the definition and sharing nothing with `oracle/` or `csrc/`: integers, one cell at a time in
meaning (one column at a time in numpy), no bit vectors.

A strip job covers columns `col0 .. col0 + n` of `a` and rows `R = 64 word0 .. 64 word0 + 32 nlanes` of `b`'s profile.

* Row codes: the kernel sees `b` only through its profile, two negated bit planes `(nb0, nb1)` per 64-row word; a row
  matches the base code `(~nb0 & 1) | (~nb1 & 1) << 1` (A0 C1 G2 T3).  Rows past `|b|` in the last word are (0, 0) and
  so match `T`: that is exactly what the GPU computes there, and the strip reports them like any other row.
* Top row: `D[0][0] = 0`, `D[0][c + 1] = D[0][c] + top[c]`, `top` from the `hin` bytes (bit0 = +1, bit1 = -1), or +1.
* Left column: `D[r + 1][0] = D[r][0] + left[r]`, `left` from the `V(p, m)` words of `v` (bit k of word w: row 64 w + k),
  or, for TAP strips given `values`, from `values` on words `[fill_word0, fill_stride)` and +1 on the others.
* Cell step: `D[r + 1][c + 1] = min(D[r][c] + [row r !~ column c], D[r][c + 1] + 1, D[r + 1][c] + 1)`.
* Outputs: `sum = D[H][n] - D[H][0]`; the right column's deltas `D[r + 1][n] - D[r][n]` as `V` words; the deltas of the
  tapped row `lane_rows * (tap + 1)` (32 rows per lane for K = 1, 64 for K = 2) as `hout` bytes.

Worked example (`rect_dp` on its own): columns `ACG`, rows `AG`, top and left all +1.

    D =  0 1 2 3        row 1 (A): A matches column 0, so D[1][1] = D[0][0] = 0
         1 0 1 2        row 2 (G): G matches column 2, so D[2][3] = D[1][2] = 1
         2 1 1 1

so `sum = D[2][3] - D[2][0] = -1`, the right column's deltas are `(-1, -1)`, the bottom row's `(-1, 0, 0)` and row 1's
`(-1, +1, +1)`.
"""
import numpy as np

_RANK = {ord(c): k for k, c in enumerate("ACGT")}
ONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def codes(seq: bytes) -> np.ndarray:
    return np.fromiter((_RANK[c] for c in seq), np.int64, len(seq))


def profile_words(b: bytes) -> np.ndarray:
    """(ceil(|b| / 64), 2) uint64: the negated bit planes (nb0, nb1) of every 64-row word; rows past |b| are (0, 0)."""
    w = (len(b) + 63) // 64
    r = np.full(64 * w, -1, np.int64)
    r[: len(b)] = codes(b)
    nb0 = np.where(r >= 0, 1 - (r & 1), 0).astype(np.uint8)
    nb1 = np.where(r >= 0, 1 - ((r >> 1) & 1), 0).astype(np.uint8)
    out = np.zeros((w, 2), np.uint64)
    out[:, 0] = np.packbits(nb0, bitorder="little").view(np.uint64)
    out[:, 1] = np.packbits(nb1, bitorder="little").view(np.uint64)
    return out


def word_bits(words: np.ndarray) -> np.ndarray:
    """uint64 array -> its bits, 64 per word, least significant first."""
    return np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little").astype(np.int64)


def row_codes(prof: np.ndarray, word0: int, nlanes: int) -> np.ndarray:
    """The base code each row of the strip matches, read back from the profile words."""
    sel = prof[word0 : word0 + nlanes // 2]
    nb0, nb1 = word_bits(sel[:, 0]), word_bits(sel[:, 1])
    return (1 - nb0) | ((1 - nb1) << 1)


def v_deltas(vw: np.ndarray) -> np.ndarray:
    """V(p, m) words -> one delta per row."""
    vw = np.asarray(vw, np.uint64).reshape(-1, 2)
    return word_bits(vw[:, 0]) - word_bits(vw[:, 1])


def v_words(d: np.ndarray) -> np.ndarray:
    """One delta per row (a multiple of 64 rows) -> V(p, m) words."""
    d = np.asarray(d, np.int64)
    out = np.zeros((len(d) // 64, 2), np.uint64)
    out[:, 0] = np.packbits((d == 1).astype(np.uint8), bitorder="little").view(np.uint64)
    out[:, 1] = np.packbits((d == -1).astype(np.uint8), bitorder="little").view(np.uint64)
    return out


def h_bytes(d: np.ndarray) -> np.ndarray:
    """Horizontal deltas -> the kernels' bytes (bit0 = +1, bit1 = -1)."""
    d = np.asarray(d, np.int64)
    return np.where(d == 1, 1, np.where(d == -1, 2, 0)).astype(np.uint8)


def h_deltas(bs: np.ndarray) -> np.ndarray:
    bs = np.asarray(bs, np.int64)
    return (bs & 1) - ((bs >> 1) & 1)


def rect_dp(col_codes, rcodes, top, left, tap_row=None):
    """D of the rectangle with columns `col_codes`, rows `rcodes`, top and left deltas -> (sum, right deltas, bottom deltas,
    deltas of row `tap_row` or None).  One column at a time: within a column the vertical +1 chain is a running minimum."""
    col_codes, rcodes = np.asarray(col_codes, np.int64), np.asarray(rcodes, np.int64)
    top, left = np.asarray(top, np.int64), np.asarray(left, np.int64)
    n, H = len(col_codes), len(rcodes)
    assert len(top) == n and len(left) == H
    idx = np.arange(H + 1, dtype=np.int64)
    col = np.concatenate([[0], np.cumsum(left)])  # D[.][0]
    first_left = col.copy()
    bottom = np.empty(n + 1, np.int64)
    tapped = np.empty(n + 1, np.int64) if tap_row is not None else None
    bottom[0] = col[H]
    if tapped is not None:
        tapped[0] = col[tap_row]
    for c in range(n):
        u = np.empty(H + 1, np.int64)
        u[0] = col[0] + top[c]
        u[1:] = np.minimum(col[:-1] + (rcodes != col_codes[c]), col[1:] + 1)
        col = idx + np.minimum.accumulate(u - idx)
        bottom[c + 1] = col[H]
        if tapped is not None:
            tapped[c + 1] = col[tap_row]
    s = int(bottom[n] - bottom[0])
    assert s == int(col[H] - col[0] - (first_left[H] - first_left[0]) + np.sum(top))
    return s, np.diff(col), np.diff(bottom), (np.diff(tapped) if tapped is not None else None)


def left_deltas(v, word0, nlanes, values=None, fill_word0=0, fill_stride=0):
    """The strip's left column: from `v`, or (TAP with `values`) from `values` inside [fill_word0, fill_stride) and +1 outside."""
    H = 32 * nlanes
    if values is None:
        return v_deltas(np.asarray(v).reshape(-1, 2)[word0 : word0 + nlanes // 2])[:H]
    out = np.ones(H, np.int64)
    vals = np.asarray(values).reshape(-1, 2)
    for k in range(nlanes // 2):
        w = word0 + k
        if fill_word0 <= w < fill_stride:
            out[64 * k : 64 * k + 64] = v_deltas(vals[w : w + 1])
    return out


def strip(job: dict, k: int = 1, tap_variant: bool = True):
    """Expected outputs of one strip job (the dict of capi.strip_probe): {"v": whole column, "hout": whole array, "sum"}.
    `k`: 64-row lanes when 2 (the tap row is 64 (tap + 1)); `tap_variant`: whether the strip writes its tapped row at all."""
    a, b = job["a"], job["b"]
    col0, n, word0, nlanes = job["col0"], job["n"], job["word0"], job["nlanes"]
    tap = job.get("tap", -1)
    hout = np.array(job["hout"], np.uint8, copy=True)
    hin = hout if job.get("hin_is_hout") else job.get("hin")
    top = np.ones(n, np.int64) if hin is None else h_deltas(np.asarray(hin)[col0 : col0 + n])
    left = left_deltas(job["v"], word0, nlanes, job.get("values"), job.get("fill_word0", 0), job.get("fill_stride", 0))
    rc = row_codes(profile_words(b), word0, nlanes)
    tap_row = (32 * k) * (tap + 1) if (tap_variant and tap >= 0) else None
    s, right, _, tapped = rect_dp(codes(a)[col0 : col0 + n], rc, top, left, tap_row)
    v = np.array(job["v"], np.uint64, copy=True).reshape(-1, 2)
    v[word0 : word0 + nlanes // 2] = v_words(right)
    if tapped is not None:
        hout[col0 : col0 + n] = h_bytes(tapped)
    return {"v": v, "hout": hout, "sum": s}
