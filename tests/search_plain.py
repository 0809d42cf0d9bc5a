"""A plain dynamic-programming reference for the semi-global search (`pa.search`, `pa.search_trace`), written from the
definition and sharing nothing with `oracle/` or `csrc/`: no bit vectors, no 64-row padding, no suffix readout.

The matrix has `plen + 1` rows (pattern) and `tlen + 1` columns (text); `D[j][i]` is the cost of the best alignment of
pattern[0..j) that ends just after text[0..i).

* Top row: `D[0][i] = 0`, the match may start anywhere in the text.
* Left column: `D[j][0] = U[j]`, the cost of leaving pattern[0..j) unmatched.  `U[j]` counts the rows `r < j` marked by
  the unmatched cost `uc`: `r = ceil(f32(i) / f32(uc))` for `i = 0, 1, 2, ...` (every `1/uc`-th row costs 1), and no row
  at all when `uc == 0`.  The arithmetic is float32 because the C ABI takes a `float`: 0.3 and 1/3 are the float32
  values, not the Python doubles.
* Cell step: `D[j][i] = min(D[j-1][i-1] + [p[j-1] !~ t[i-1]], D[j-1][i] + 1, D[j][i-1] + 1)`, where `!~` means
  incompatible.  Pattern letters: ACGT, N and * (any), Y (C or T), R (A or G), either case.  Text letters: ACGT, either
  case.
* Output: the bottom row `out[i] = D[plen][i]` for `i = 0..tlen`, then the right column upwards,
  `out[tlen + t] = D[plen - t][tlen] + U[plen] - U[plen - t]` for `t = 1..plen`: an alignment that ends in row
  `plen - t` leaves the last `t` pattern rows unmatched, at the unmatched cost of those rows.

Why this is what the bit-parallel search computes: it pads the pattern to a multiple of 64 rows with rows that match
everything and no unmatched-cost marks.  A wildcard row only shifts the row above it one column to the right,
`D_pad[plen + p][c] = D[plen][c - p]` for `c >= p`, and its left column stays `U[plen]`.  The padded readout walks the
bottom padded row and then the right column upwards and drops the first `padding` values after `out[0]`; what it keeps
are exactly `D[plen][0..tlen]` followed by rows `plen - 1 .. 0` of the last column, whether the dropped values come from
the bottom row alone or, when `tlen < padding`, partly from the padding rows of the right column.

Hand checks against the two answers the reference documents:

* `AC` in `CTTACTTA`, `uc = 0`: `U = 0`.  Row 1 (`A`) is `0 1 1 1 0 1 1 1 0`, row 2 (`C`) is `0 0 1 2 1 0 1 2 1`;
  the right column upwards is `D[1][8] = 0` and `D[0][8] = 0`, so `out = [0,0,1,2,1,0,1,2,1,0,0]`.
* `CT` in `ACTG`, `uc = 1`: rows 0 and 1 are marked, `U = [0, 1, 2]`.  Row 1 (`C`) is `1 1 0 1 1`, row 2 (`T`) is
  `2 2 1 0 1`; the right column adds `D[1][4] + 2 - 1 = 2` and `D[0][4] + 2 - 0 = 2`, so `out = [2,2,1,0,1,2,2]`.

`check_trace` verifies a traced alignment on its own terms.  Together with `out == search(...)` it proves the alignment
optimal without relying on any restatement of the reference's traceback.
"""
import re

import numpy as np

_TEXT_CODE = {ord(c): k for k, c in enumerate("ACGT")} | {ord(c): k for k, c in enumerate("acgt")}
_PATTERN_SET = {"A": "A", "C": "C", "G": "G", "T": "T", "N": "ACGT", "*": "ACGT", "Y": "CT", "R": "AG"}
_PATTERN_MASK = {}
for _c, _s in _PATTERN_SET.items():
    _m = sum(1 << "ACGT".index(x) for x in _s)
    _PATTERN_MASK[ord(_c)] = _m
    _PATTERN_MASK[ord(_c.lower())] = _m


def text_codes(text: bytes) -> np.ndarray:
    try:
        return np.fromiter((_TEXT_CODE[c] for c in text), np.int8, len(text))
    except KeyError as e:
        raise ValueError(f"text letter {chr(e.args[0])!r}") from None


def pattern_masks(pattern: bytes) -> list[int]:
    try:
        return [_PATTERN_MASK[c] for c in pattern]
    except KeyError as e:
        raise ValueError(f"pattern letter {chr(e.args[0])!r}") from None


def compatible(p: int, t: int) -> bool:
    """Pattern letter p and text letter t (byte values) match."""
    return bool((_PATTERN_MASK[p] >> _TEXT_CODE[t]) & 1)


def unmatched_prefix(plen: int, uc: float) -> np.ndarray:
    """U[0..plen]: how many of the rows 0..j-1 cost 1 when left unmatched (float32 arithmetic, as the C ABI's float)."""
    marks = np.zeros(plen, np.int64)
    uc32 = np.float32(uc)
    if uc32 > 0 and plen > 0:
        # ceil(f32(i) / uc) is non-decreasing in i and at least i (uc <= 1): the rows below plen come from i < plen.
        i = np.arange(plen, dtype=np.float32)
        rows = np.ceil(i / uc32)
        marks[rows[rows < plen].astype(np.int64)] = 1
    return np.concatenate([[0], np.cumsum(marks)])


def search(pattern: bytes, text: bytes, uc: float) -> list[int]:
    """out[0 .. plen + tlen] by the row-by-row DP above.  Row j's horizontal +1 chain is a running minimum:
    E[i] = min_k<=i (C[k] + i - k) = i + min.accumulate(C - i)."""
    plen, tlen = len(pattern), len(text)
    t = text_codes(text)
    masks = pattern_masks(pattern)
    U = unmatched_prefix(plen, uc)
    ramp = np.arange(tlen + 1, dtype=np.int32)
    mismatch = {m: ((m >> t.astype(np.int32)) & 1 ^ 1).astype(np.int32) for m in set(masks)}
    row = np.zeros(tlen + 1, np.int32)
    right = [int(row[tlen])]
    c = np.empty(tlen + 1, np.int32)
    for j in range(1, plen + 1):
        c[0] = U[j]
        np.minimum(row[:-1] + mismatch[masks[j - 1]], row[1:] + 1, out=c[1:])
        c -= ramp
        row = np.minimum.accumulate(c) + ramp
        right.append(int(row[tlen]))
    out = row.tolist()
    out += [right[plen - k] + int(U[plen] - U[plen - k]) for k in range(1, plen + 1)]
    return out


def idx_to_pos(plen: int, tlen: int, idx: int) -> tuple[int, int]:
    """Output index -> (text index, pattern index): the bottom row left to right, then the right column upwards."""
    return (idx, plen) if idx <= tlen else (tlen, plen - (idx - tlen))


def cigar_ops(cigar: str) -> str:
    parts = re.findall(r"(\d*)([=XID])", cigar)
    assert "".join(n + op for n, op in parts) == cigar, f"malformed CIGAR {cigar!r}"
    return "".join(op * (int(n) if n else 1) for n, op in parts)


_STEP = {"=": (1, 1), "X": (1, 1), "D": (1, 0), "I": (0, 1)}


def check_trace(pattern: bytes, text: bytes, uc: float, idx: int, out, cigar: str, path) -> None:
    """Assert that (cigar, path) is an alignment ending at output index idx whose cost is out[idx]:

    * the path is a monotone walk inside the matrix that ends at idx_to_pos(idx) and starts in column 0 or row 0;
    * its steps spell the CIGAR (= and X diagonal, D a text step, I a pattern step), = on compatible letters and X on
      incompatible ones;
    * out[idx] = #X + #I + #D + U[start row] (if it starts in column 0) + U[plen] - U[end row].
    """
    plen, tlen = len(pattern), len(text)
    U = unmatched_prefix(plen, uc)
    ops = cigar_ops(cigar)
    path = [tuple(p) for p in path]
    assert len(path) == len(ops) + 1, (len(path), len(ops))
    assert path[-1] == idx_to_pos(plen, tlen, idx), (path[-1], idx)
    i0, j0 = path[0]
    assert 0 <= i0 <= tlen and 0 <= j0 <= plen and (i0 == 0 or j0 == 0), path[0]
    for k, op in enumerate(ops):
        (i, j), (i1, j1) = path[k], path[k + 1]
        assert (i1 - i, j1 - j) == _STEP[op], (k, op, path[k], path[k + 1])
        if op in "=X":
            assert compatible(pattern[j], text[i]) == (op == "="), (k, op, chr(pattern[j]), chr(text[i]))
    edits = len(ops) - ops.count("=")
    j_end = path[-1][1]
    cost = edits + (int(U[j0]) if i0 == 0 else 0) + int(U[plen] - U[j_end])
    assert cost == out[idx], (cost, out[idx], idx)
