"""Plain diagonal transition (WFA) with free text ends, the test oracle of AffineBatch.run_dt_ends / align_dt_ends: tests/affine_dt_plain.py's
fronts, recurrence, extension and walk with the two switches of tests/affine_ends_plain.py.  a is the text, b the pattern, consumed whole.

  free_start  front 0 starts every diagonal k = 0 .. |a| at (k, 0): the value before extension is k.  The live diagonals of cost s are
              [-min(|b|, reach_ins(s)), |a|].  Without it front 0 is diagonal 0 at 0 and the range is affine_dt's.
  free_end    the pair is found at the first s at which some diagonal holds M_s[k] - k = |b|; `end` is the lowest such i = M_s[k] (the
              lowest k: the DP's lowest column on ties).  Without it the test is M_s[|a| - |b|] = |a| and end = |a|.
  bound       with either switch on, min(s_max, the gap cost of inserting b): end = 0, or start = |a|, is always a path.

The walk starts at (cost, main, i = end, k = end - |b|) with affine_dt's parent order and tie rule and ends at s = 0, where it emits
i - k matches; start = k under free_start, else k is 0 and so is start.  The CIGAR describes a[start:end] against b.  Cost and end are
those of affine_ends; start and the CIGAR are this walk's own and may be another optimal placement.  Above s_max: (-1, -1, -1, "").
With both switches off this is affine_dt with start = 0 and end = |a|.
"""
from __future__ import annotations

import numpy as np

from tests.affine_dt_plain import NEG, _Fronts, gap_cost, reach
from tests.affine_plain import cigar_text, edge_costs


def affine_dt_ends(a: bytes, b: bytes, cm, s_max: int, free_start: bool = False, free_end: bool = False):
    """-> (cost, start, end, CIGAR), or (-1, -1, -1, "") when the cost exceeds s_max."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8)
    B = np.frombuffer(b, np.uint8)
    sub, ins, dl, io, ie, do, de = edge_costs(cm)
    if free_start or free_end:
        s_max = min(s_max, gap_cost(m, ins, io, ie))
    else:
        s_max = min(s_max, gap_cost(n, dl, do, de) + gap_cost(m, ins, io, ie))
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

    cost = end = -1
    for s in range(s_max + 1):
        klo = -min(m, reach(s, ins, io, ie))
        khi = n if free_start else min(n, reach(s, dl, do, de))
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
            pre = k.copy() if free_start else np.zeros(1, np.int64)  # (the live range of cost 0 is [0, |a|], or diagonal 0)
        Ms = extend(pre, k)
        M.put(klo, Ms)
        if free_end:
            hit = np.nonzero(Ms - k == m)[0]
            if len(hit):
                cost, end = s, int(Ms[hit[0]])
                break
        elif klo <= n - m <= khi and M.at(s, n - m) == n:
            cost, end = s, n
            break
    if cost < 0:
        return -1, -1, -1, ""

    # the walk
    ops = []  # from the end
    s, layer, k, i = cost, 0, end - m, end
    while True:
        if layer == 0:
            if s == 0:
                assert free_start or k == 0
                ops += ["="] * (i - k)
                start = k
                break
            assert not (free_start and i == k), "on row 0 at positive cost"
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
    return cost, start, end, cigar_text(ops[::-1])
