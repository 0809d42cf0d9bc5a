"""Plain DP of the ends-free (semi-global) mode of the batched gap-affine aligner (AffineBatch.set_free_ends), the oracle of its tests.

tests/affine_plain.affine_nw's anti-diagonal numpy DP with two switches on a, the text (columns); b, the pattern (rows), is always
consumed whole:
  free_start  M(i, 0) = 0 for every i (I(i, 0) stays absent; row 0's D feeds only row 0's M, so it does not matter);
  free_end    the cost is the minimum of M(i, |b|) over i = 0 .. |a|, `end` the lowest i that reaches it; without it end = |a|.
The traceback is affine_nw's first-parent walk over the same code bytes, from (end, |b|, main); with free_start it stops at the first
state (i, 0, main) it reaches and start = i, else it runs to (0, 0, main) and start = 0.  The CIGAR describes a[start:end] against b.
With both switches off this is affine_nw.
"""
from __future__ import annotations

import numpy as np

from tests.affine_plain import INF, cigar_text, edge_costs


def affine_ends(a: bytes, b: bytes, cm, free_start: bool = False, free_end: bool = False, trace: bool = True):
    """-> (cost, start, end, CIGAR, last_row); start and CIGAR are None without trace.  last_row: int64[|a| + 1], M(i, |b|)."""
    if len(cm.layers) > 2 or [k for k, _, _ in cm.layers] not in ([], ["ins", "del"]):
        raise ValueError("N in {0, 2} only")
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8).astype(np.int64)
    B = np.frombuffer(b, np.uint8).astype(np.int64)
    big = 4 * INF  # an absent edge: never below INF
    sub, ins, dl, io, ie, do, de = [big if c is None else int(c) for c in edge_costs(cm)]
    codes = np.zeros((n + 1, m + 1), np.uint8) if trace else None
    last_row = np.zeros(n + 1, np.int64)
    full = lambda: np.full(n + 1, INF, np.int64)  # noqa: E731  a diagonal, indexed by i
    M2, M1, I1, D1 = full(), full(), full(), full()
    for d in range(n + m + 1):
        i = np.arange(max(0, d - m), min(n, d) + 1)
        j = d - i
        up, left, dg = j >= 1, i >= 1, (i >= 1) & (j >= 1)
        im1 = np.maximum(i - 1, 0)
        Mup = np.where(up, M1[i], INF)
        Iup = np.where(up, I1[i], INF)
        Mleft = np.where(left, M1[im1], INF)
        Dleft = np.where(left, D1[im1], INF)
        Mdiag = np.where(dg, M2[im1], INF)
        eq = dg & (A[im1] == B[np.maximum(j - 1, 0)]) if n and m else np.zeros(len(i), bool)
        iop, iex = Mup + io, Iup + ie
        I = np.minimum(np.minimum(iop, iex), INF)
        dop, dex = Mleft + do, Dleft + de
        D = np.minimum(np.minimum(dop, dex), INF)
        cand = [np.where(dg, Mdiag + np.where(eq, 0, sub), big), Mup + ins, Mleft + dl, I + ie, D + de]
        M = np.minimum.reduce(cand + [np.full(len(i), INF, np.int64)])
        if d == 0:
            M[:] = 0
        if free_start and d <= n:
            M[j == 0] = 0  # the cell (d, 0)
        if trace:
            c = np.full(len(i), 4, np.uint8)
            for k in (3, 2, 1, 0):
                c = np.where(M == cand[k], np.uint8(k), c)
            c = c | np.where(I == iop, 0, 8).astype(np.uint8) | np.where(D == dop, 0, 16).astype(np.uint8)
            codes[i, j] = c
        if d >= m:
            last_row[d - m] = M[0]  # i = d - m is the diagonal's first cell
        nM, nI, nD = full(), full(), full()
        nM[i], nI[i], nD[i] = M, I, D
        M2, M1, I1, D1 = M1, nM, nI, nD
    end = int(np.argmin(last_row)) if free_end else n  # argmin: the first, i.e. lowest, minimiser
    cost = int(last_row[end])
    if not trace:
        return cost, None, end, None, last_row
    start, cigar = _walk(a, b, codes, end, free_start)
    return cost, start, end, cigar, last_row


def _walk(a, b, codes, end, free_start):
    i, j, layer = end, len(b), 0
    ops = []  # from the end: '=', 'X', 'I', 'D' (linear), 'i', 'd' (affine)
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
    return i, cigar_text(ops[::-1])
