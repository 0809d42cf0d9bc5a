"""Plain DP of the ends-free (semi-global) mode of the batched double-affine aligner (Affine4Batch.set_free_ends), the oracle of its
tests.

tests/affine4_plain.affine4_nw's anti-diagonal numpy DP with two switches on a, the text (columns); b, the pattern (rows), is always
consumed whole:
  free_start  M(i, 0) = 0 for every i (I1(i, 0) and I2(i, 0) stay absent; row 0's D1 and D2 feed only row 0's M, so they do not matter);
  free_end    the cost is the minimum of M(i, |b|) over i = 0 .. |a|, `end` the lowest i that reaches it; without it end = |a|.
The traceback is affine4_nw's first-parent walk over the same code bytes, from (end, |b|, main); with free_start it stops at the first
state (i, 0, main) it reaches and start = i, else it runs to (0, 0, main) and start = 0.  The CIGAR describes a[start:end] against b;
gaps of different layers, and linear against affine, stay separate elements.  With both switches off this is affine4_nw.
"""
from __future__ import annotations

import numpy as np

from tests.affine4_plain import INF, _LAYER_OPS, _model


def affine4_ends(a: bytes, b: bytes, cm, free_start: bool = False, free_end: bool = False, trace: bool = True):
    """-> (cost, start, end, CIGAR, last_row); start and CIGAR are None without trace.  last_row: int64[|a| + 1], M(i, |b|)."""
    sub, ins, dl, op, ex = _model(cm)
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8).astype(np.int64)
    B = np.frombuffer(b, np.uint8).astype(np.int64)
    big = 4 * INF  # an absent edge: never below INF
    sub, ins, dl = [big if c is None else int(c) for c in (sub, ins, dl)]
    codes = np.zeros((n + 1, m + 1), np.uint8) if trace else None
    last_row = np.zeros(n + 1, np.int64)
    full = lambda: np.full(n + 1, INF, np.int64)  # noqa: E731  a diagonal, indexed by i
    M2, M1 = full(), full()
    L1 = [full() for _ in range(4)]
    for d in range(n + m + 1):
        i = np.arange(max(0, d - m), min(n, d) + 1)
        j = d - i
        up, left, dg = j >= 1, i >= 1, (i >= 1) & (j >= 1)
        im1 = np.maximum(i - 1, 0)
        Mup = np.where(up, M1[i], INF)
        Mleft = np.where(left, M1[im1], INF)
        Mdiag = np.where(dg, M2[im1], INF)
        eq = dg & (A[im1] == B[np.maximum(j - 1, 0)]) if n and m else np.zeros(len(i), bool)
        lay, opened = [], []
        for k in range(4):  # insert layers come from (i, j-1), delete layers from (i-1, j)
            if k % 2 == 0:
                o_, e_ = Mup + op[k] + ex[k], np.where(up, L1[k][i], INF) + ex[k]
            else:
                o_, e_ = Mleft + op[k] + ex[k], np.where(left, L1[k][im1], INF) + ex[k]
            lay.append(np.minimum(np.minimum(o_, e_), INF))
            opened.append(o_)
        cand = [np.where(dg, Mdiag + np.where(eq, 0, sub), big), Mup + ins, Mleft + dl] + lay
        M = np.minimum.reduce(cand + [np.full(len(i), INF, np.int64)])
        if d == 0:
            M[:] = 0
        if free_start and d <= n:
            M[j == 0] = 0  # the cell (d, 0)
        if trace:
            c = np.full(len(i), 6, np.uint8)
            for k in (5, 4, 3, 2, 1, 0):
                c = np.where(M == cand[k], np.uint8(k), c)
            for k in range(4):
                c = c | np.where(lay[k] == opened[k], 0, 8 << k).astype(np.uint8)
            codes[i, j] = c
        if d >= m:
            last_row[d - m] = M[0]  # i = d - m is the diagonal's first cell
        nM = full()
        nM[i] = M
        nL = [full() for _ in range(4)]
        for k in range(4):
            nL[k][i] = lay[k]
        M2, M1, L1 = M1, nM, nL
    end = int(np.argmin(last_row)) if free_end else n  # argmin: the first, i.e. lowest, minimiser
    cost = int(last_row[end])
    if not trace:
        return cost, None, end, None, last_row
    start, cigar = _walk(a, b, codes, end, free_start)
    return cost, start, end, cigar, last_row


def _walk(a, b, codes, end, free_start):
    i, j, layer = end, len(b), 0  # layer: 0 main, 1 + k for layer k
    ops = []
    while not (j == 0 and layer == 0 and (free_start or i == 0)):
        c = int(codes[i, j])
        if layer == 0:
            k = c & 7
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
                assert k <= 6
                layer = k - 2
        else:
            k = layer - 1
            ops.append(_LAYER_OPS[k])
            if k % 2:
                i -= 1
            else:
                j -= 1
            if not c & (8 << k):
                layer = 0
        assert i >= 0 and j >= 0
    out = []
    for o in ops[::-1]:
        if out and out[-1][0] == o:
            out[-1][1] += 1
        else:
            out.append([o, 1])
    return i, "".join(("" if k == 1 else str(k)) + {"i": "I", "j": "I", "d": "D", "e": "D"}.get(o, o) for o, k in out)
