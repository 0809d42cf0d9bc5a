"""Plain diagonal transition (WFA) over the gap-affine edit graph of tests/affine_plain.py, the test oracle of the batched DT route
(AffineBatch.run_dt / align_dt).

Diagonal k holds the states with i - j = k (i in a, j in b).  For every cost s and layer (main, insert, delete) a front keeps the
furthest-reaching i of every diagonal, NEG where the layer does not reach the diagonal at that cost.  The edges are those of the edit
graph: a substitution keeps k and advances i; an insertion (linear, or open / extend of the insert layer) goes from k + 1 to k at the same
i; a deletion goes from k - 1 to k and advances i; closing a layer costs `extend` and moves nothing.  Matches are free, so the main
layer is extended along them after every step.  The pair is found at the first s whose main layer reaches (|a|, |b|); with no such
s <= s_max it is not found: (-1, "").

The walk back, from (cost, main, |a|, |b|): on the main layer the point before extension is the maximum over the parents in the order
substitution, linear insert, linear delete, close insert, close delete; the matches down to it are emitted and the walk moves to the
first parent that reaches it.  On an affine layer open comes before extend.  At s = 0 the rest is all matches.
"""
from __future__ import annotations

import numpy as np

from tests.affine_plain import cigar_text, edge_costs

NEG = -(1 << 30)


def reach(s: int, lin, op, ex) -> int:
    """The longest gap that cost s pays for on any layer: L lin <= s on the main layer, op + (L - 1) ex <= s on the affine layer (which
    is `ex` short of closing)."""
    r = 0
    if lin is not None:
        r = s // lin
    if op is not None and s >= op:
        r = max(r, (s - op) // ex + 1)
    return r


def gap_cost(L: int, lin, op, ex) -> int:
    if L == 0:
        return 0
    return min(([L * lin] if lin is not None else []) + ([op + L * ex] if op is not None else []))


class _Fronts:
    """Fronts of one layer: per cost an array over the live diagonals [lo, hi] of that cost."""

    def __init__(self):
        self.f = []  # (lo, array)

    def put(self, lo, arr):
        self.f.append((lo, arr))

    def get(self, s, klo, khi):
        """Values of front s on diagonals klo .. khi, NEG outside what it holds (and for s < 0)."""
        out = np.full(khi - klo + 1, NEG, np.int64)
        if s < 0:
            return out
        lo, arr = self.f[s]
        x0, x1 = max(klo, lo), min(khi, lo + len(arr) - 1)
        if x0 <= x1:
            out[x0 - klo:x1 - klo + 1] = arr[x0 - lo:x1 - lo + 1]
        return out

    def at(self, s, k):
        return int(self.get(s, k, k)[0])


def affine_dt(a: bytes, b: bytes, cm, s_max: int):
    """-> (cost, CIGAR), or (-1, "") when the cost exceeds s_max."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8)
    B = np.frombuffer(b, np.uint8)
    sub, ins, dl, io, ie, do, de = edge_costs(cm)
    s_max = min(s_max, gap_cost(n, dl, do, de) + gap_cost(m, ins, io, ie))  # deleting a and inserting b is always a path
    M, I, D = _Fronts(), _Fronts(), _Fronts()

    def valid(v, k):
        return np.where((v >= 0) & (v <= n) & (v - k >= 0) & (v - k <= m), v, NEG)

    def extend(v, k):
        v = v.copy()
        while True:
            j = v - k
            live = (v >= 0) & (v < n) & (j < m)
            hit = np.zeros(len(v), bool)
            hit[live] = A[v[live]] == B[j[live]]
            if not hit.any():
                return v
            v[hit] += 1

    cost = -1
    for s in range(s_max + 1):
        klo, khi = -min(m, reach(s, ins, io, ie)), min(n, reach(s, dl, do, de))
        k = np.arange(klo, khi + 1)
        neg = np.full(len(k), NEG, np.int64)
        Iv = Dv = neg
        if io is not None:
            Iv = valid(np.maximum(M.get(s - io, klo + 1, khi + 1), I.get(s - ie, klo + 1, khi + 1)), k)
        if do is not None:
            Dv = valid(np.maximum(M.get(s - do, klo - 1, khi - 1), D.get(s - de, klo - 1, khi - 1)) + 1, k)
        I.put(klo, Iv)
        D.put(klo, Dv)
        c = [neg] * 5
        if sub is not None:
            c[0] = valid(M.get(s - sub, klo, khi) + 1, k)
        if ins is not None:
            c[1] = valid(M.get(s - ins, klo + 1, khi + 1), k)
        if dl is not None:
            c[2] = valid(M.get(s - dl, klo - 1, khi - 1) + 1, k)
        if io is not None:
            c[3] = I.get(s - ie, klo, khi)
        if do is not None:
            c[4] = D.get(s - de, klo, khi)
        pre = np.maximum.reduce(c)
        if s == 0:
            pre = np.zeros(1, np.int64)
        M.put(klo, extend(pre, k))
        if klo <= n - m <= khi and M.at(s, n - m) == n:
            cost = s
            break
    if cost < 0:
        return -1, ""

    # the walk
    ops = []  # from the end
    s, layer, k, i = cost, 0, n - m, n
    while True:
        if layer == 0:
            if s == 0:
                assert k == 0
                ops += ["="] * i
                break
            par = [
                (M.at(s - sub, k) + 1, 0, sub, k, "X") if sub is not None else None,
                (M.at(s - ins, k + 1), 0, ins, k + 1, "I") if ins is not None else None,
                (M.at(s - dl, k - 1) + 1, 0, dl, k - 1, "D") if dl is not None else None,
                (I.at(s - ie, k), 1, ie, k, None) if io is not None else None,
                (D.at(s - de, k), 2, de, k, None) if do is not None else None,
            ]
            par = [q for q in par if q is not None and 0 <= q[0] <= n and 0 <= q[0] - k <= m]
            pre = max(q[0] for q in par)
            assert pre <= i
            ops += ["="] * (i - pre)
            v, layer, c, k2, op = next(q for q in par if q[0] == pre)
            if op is not None:
                ops.append(op)
            i = pre - (1 if op in ("X", "D") else 0)
            s, k = s - c, k2
        elif layer == 1:
            ops.append("I")
            if M.at(s - io, k + 1) == i:
                s, layer = s - io, 0
            else:
                assert I.at(s - ie, k + 1) == i
                s = s - ie
            k += 1
        else:
            ops.append("D")
            if M.at(s - do, k - 1) + 1 == i:
                s, layer = s - do, 0
            else:
                assert D.at(s - de, k - 1) + 1 == i
                s = s - de
            k, i = k - 1, i - 1
    return cost, cigar_text(ops[::-1])
