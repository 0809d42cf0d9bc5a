"""Plain restatement of local (Smith-Waterman) alignment under a gap-affine cost model and a bonus per match, the test oracle of
pa_affine_batch_run_local / pa_affine_batch_align_local (include/pa_affine_local_hip.h has the definition).

The DP runs over anti-diagonals with numpy, like affine_plain.py, in signed scores: per cell the affine layers before the main layer,
    I(i,j) = max(H(i,j-1) - ins_open, I(i,j-1) - ins_extend)
    D(i,j) = max(H(i-1,j) - del_open, D(i-1,j) - del_extend)
    H(i,j) = max(0, H(i-1,j-1) + (match or -sub), H(i,j-1) - ins, H(i-1,j) - del, I(i,j) - ins_extend, D(i,j) - del_extend)
with H = 0 and I, D absent on row 0 and column 0.  The answer is the highest H, at the lowest i and then the lowest j; the walk goes
from there by the first parent that fits (diagonal, linear insertion, linear deletion, close of the insert layer, close of the delete
layer; in the layers open before extend) until a main-layer state with H = 0.  The code byte is affine_plain's with main value 5 = stop.
"""
from __future__ import annotations

import numpy as np

from tests.affine_plain import cigar_elems, cigar_text, edge_costs

NEG = -(1 << 40)  # an absent state or edge: no reachable state holds it, and it never wins against the floor at 0
STOP = 5


def local_sw(a: bytes, b: bytes, cm, match: int, trace: bool = True):
    """-> (score, cigar, a_start, a_end, b_start, b_end); with trace=False cigar, a_start and b_start are None."""
    if len(cm.layers) > 2 or [k for k, _, _ in cm.layers] not in ([], ["ins", "del"]):
        raise ValueError("N in {0, 2} only")
    if isinstance(match, bool) or not isinstance(match, (int, np.integer)) or not 1 <= match <= 1000:
        raise ValueError("match in [1, 1000]")
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8).astype(np.int64)
    B = np.frombuffer(b, np.uint8).astype(np.int64)
    big = 1 << 42  # an absent edge
    sub, ins, dl, io, ie, do, de = [big if c is None else int(c) for c in edge_costs(cm)]
    H = np.zeros((n + 1, m + 1), np.int64)
    codes = np.full((n + 1, m + 1), STOP, np.uint8)
    neg = lambda: np.full(n + 1, NEG, np.int64)  # noqa: E731  a diagonal, indexed by i
    H2, H1, I1, D1 = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), neg(), neg()
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)  # cells with i >= 1 and j >= 1
        nH, nI, nD = np.zeros(n + 1, np.int64), neg(), neg()
        if len(i):
            j = d - i
            eq = A[i - 1] == B[j - 1]
            Hup, Iup = H1[i], I1[i]  # (i, j - 1)
            Hleft, Dleft = H1[i - 1], D1[i - 1]  # (i - 1, j)
            iop, iex = Hup - io, Iup - ie
            I = np.maximum(iop, iex)
            dop, dex = Hleft - do, Dleft - de
            D = np.maximum(dop, dex)
            cand = [H2[i - 1] + np.where(eq, match, -sub), Hup - ins, Hleft - dl, I - ie, D - de]
            h = np.maximum.reduce(cand + [np.zeros(len(i), np.int64)])
            c = np.full(len(i), 4, np.uint8)
            for k in (3, 2, 1, 0):
                c = np.where(h == cand[k], np.uint8(k), c)
            c = np.where(h == 0, np.uint8(STOP), c)
            c = c | np.where(I == iop, 0, 8).astype(np.uint8) | np.where(D == dop, 0, 16).astype(np.uint8)
            H[i, j] = h
            codes[i, j] = c
            nH[i], nI[i], nD[i] = h, I, D
        H2, H1, I1, D1 = H1, nH, nI, nD
    score = int(H.max())
    if score == 0:
        a_end = b_end = 0
    else:
        a_end, b_end = (int(x) for x in np.argwhere(H == score)[0])  # row-major: the lowest i, then the lowest j
    if not trace:
        return score, None, None, a_end, None, b_end
    cigar, a_start, b_start = _walk(a, b, H, codes, a_end, b_end)
    return score, cigar, a_start, a_end, b_start, b_end


def _walk(a, b, H, codes, i, j):
    layer = 0
    ops = []  # from the end: '=', 'X', 'I', 'D' (linear), 'i', 'd' (affine)
    while True:
        c = int(codes[i, j])
        if layer == 0:
            if H[i, j] == 0:
                assert i == 0 or j == 0 or c & 7 == STOP
                break
            k = c & 7
            assert k != STOP
            if k == 0:
                ops.append("=" if a[i - 1] == b[j - 1] else "X")
                i, j = i - 1, j - 1
            elif k == 1:
                ops.append("I")
                j -= 1
            elif k == 2:
                ops.append("D")
                i -= 1
            else:
                layer = k - 2
        elif layer == 1:
            ops.append("i")
            j -= 1
            layer = 1 if c & 8 else 0
        else:
            ops.append("d")
            i -= 1
            layer = 2 if c & 16 else 0
        assert i >= 0 and j >= 0
    return cigar_text(ops[::-1]), i, j


def local_verify(cigar: str, a: bytes, b: bytes, a_start: int, b_start: int, cm, match: int):
    """Price a CIGAR on its own, from (a_start, b_start): '=' must match and scores match, 'X' must differ and scores -sub, a run of L
    'I' scores -min(L ins, open + L extend) over the edges that exist, likewise 'D'.  -> (score, a_end, b_end)."""
    sub, ins, dl, io, ie, do, de = edge_costs(cm)
    i, j, score = a_start, b_start, 0
    for k, op in cigar_elems(cigar):
        assert k >= 1
        if op in "=X":
            for _ in range(k):
                assert i < len(a) and j < len(b), "CIGAR runs past a sequence"
                if op == "=":
                    assert a[i] == b[j], f"'=' on {a[i]} != {b[j]}"
                    score += match
                else:
                    assert a[i] != b[j] and sub is not None, "'X' on equal bytes or without sub"
                    score -= sub
                i, j = i + 1, j + 1
        else:
            lin, op_, ex = (ins, io, ie) if op == "I" else (dl, do, de)
            opts = ([k * lin] if lin is not None else []) + ([op_ + k * ex] if op_ is not None else [])
            assert opts, f"no edge for {op}"
            score -= min(opts)
            if op == "I":
                j += k
            else:
                i += k
    assert i <= len(a) and j <= len(b), "CIGAR runs past a sequence"
    return score, i, j
