"""Plain diagonal transition (WFA) over the four-layer edit graph of tests/affine4_plain.py (layers [ins, del, ins, del]), global and with
free text ends: the test oracle of Affine4Batch.run_dt / align_dt / run_dt_ends / align_dt_ends, and the definition they are held to byte
for byte.  tests/affine_dt_plain.py and tests/affine_dt_ends_plain.py restated for five layers.

Diagonal k holds the states with i - j = k (i in a, j in b).  For every cost s a front keeps the furthest-reaching i of every diagonal,
for the main layer and each of layers 0 .. 3, NEG where the layer does not reach the diagonal at that cost.  Opening layer t costs
open_t and consumes a byte, extending costs extend_t and consumes one, closing costs extend_t and consumes nothing, so a gap of length L
in layer t costs open_t + L extend_t.  With x the front `s - edge cost`:
  L_t,s[k] = max(M_x[k + 1], L_t,x[k + 1])        t = 0, 2 (insert: from diagonal k + 1 at the same i)
  L_t,s[k] = max(M_x[k - 1], L_t,x[k - 1]) + 1    t = 1, 3 (delete: from diagonal k - 1, i advances)
  M_s[k]   = extend(max(M_x[k] + 1, M_x[k + 1], M_x[k - 1] + 1, L_0,x[k], L_1,x[k], L_2,x[k], L_3,x[k]))
A candidate outside the matrix is absent; an absent sub / ins / del is no edge.  The bound is min(s_max, cost of deleting a and inserting
b), a gap priced by the cheapest of the linear edge and the two pieces.  Global: found at the first s with M_s[|a| - |b|] = |a|.

  free_start  front 0 starts every diagonal k = 0 .. |a| at (k, 0); the live diagonals of cost s are [-min(|b|, reach_ins(s)), |a|].
  free_end    found at the first s at which some diagonal holds M_s[k] - k = |b|; `end` is the lowest such diagonal's M_s[k].
  bound       with either switch on, min(s_max, the cost of inserting b).

The walk starts at (cost, main, i = end, k = end - |b|).  On the main layer the parents come in iterate_parents order: substitution,
linear insert, linear delete, close of layer 0, 1, 2, 3; the point before extension is the maximum over them, the matches down to it are
emitted and the walk moves to the first parent that reaches it.  Inside a layer open comes before extend.  At s = 0 it emits i - k
matches and start = k.  Steps of different layers are distinct ops (affine4_plain._LAYER_OPS), merged only when equal, and print as I / D.
Not found: (-1, "", -1, -1).
"""
from __future__ import annotations

import numpy as np

from tests.affine4_plain import _LAYER_OPS, _model
from tests.affine4_plain import gap_cost as _w
from tests.affine_dt_plain import NEG, _Fronts

_PRINT = {"i": "I", "j": "I", "d": "D", "e": "D"}


def ins_cost(L: int, cm) -> int:
    _, ins, _, op, ex = _model(cm)
    return 0 if L == 0 else _w(L, ins, [(op[0], ex[0]), (op[2], ex[2])])


def del_cost(L: int, cm) -> int:
    _, _, dl, op, ex = _model(cm)
    return 0 if L == 0 else _w(L, dl, [(op[1], ex[1]), (op[3], ex[3])])


def reach(s: int, lin, pieces) -> int:
    """The longest gap that cost s pays for on any layer of one direction: L lin <= s on the main layer, open + (L - 1) extend <= s
    inside a layer (which is `extend` short of closing)."""
    r = s // lin if lin is not None else 0
    for o, e in pieces:
        if s >= o:
            r = max(r, (s - o) // e + 1)
    return r


def bound_of(n: int, m: int, cm, s_max: int, free_start: bool, free_end: bool) -> int:
    return min(s_max, (0 if free_start or free_end else del_cost(n, cm)) + ins_cost(m, cm))


def live_range(s: int, n: int, m: int, cm, free_start: bool):
    _, ins, dl, op, ex = _model(cm)
    klo = -min(m, reach(s, ins, [(op[0], ex[0]), (op[2], ex[2])]))
    khi = n if free_start else min(n, reach(s, dl, [(op[1], ex[1]), (op[3], ex[3])]))
    return klo, khi


def mean_w(pairs, cm, s_max, fs=False, fe=False):
    """The mean W of a batch by the host's rule (csrc/affine4_dt_plan.hpp shape_of, restated); its blocks are wide where this exceeds 256."""
    _, ins, _, op, ex = _model(cm)
    ws = []
    for a, b in pairs:
        n, m = len(a), len(b)
        sb = bound_of(n, m, cm, s_max, fs, fe)
        back = reach(sb, ins, [(op[0], ex[0]), (op[2], ex[2])])
        kmax = min(n, max(0, n - m + back)) if fs else live_range(sb, n, m, cm, False)[1]
        ws.append(kmax + min(m, back) + 3)
    return sum(ws) / len(ws)


def cigar_text(ops) -> str:
    out = []
    for op in ops:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return "".join(("" if k == 1 else str(k)) + _PRINT.get(op, op) for op, k in out)


def affine4_dt(a: bytes, b: bytes, cm, s_max: int, free_start: bool = False, free_end: bool = False, raw: bool = False):
    """-> (cost, CIGAR, start, end), or (-1, "", -1, -1) when the cost exceeds s_max; with raw the walk's ops before printing, one
    character a step (affine4_plain.affine4_nw), in place of the CIGAR."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8)
    B = np.frombuffer(b, np.uint8)
    sub, ins, dl, op, ex = _model(cm)
    s_max = bound_of(n, m, cm, s_max, free_start, free_end)
    M = _Fronts()
    Ls = [_Fronts() for _ in range(4)]

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
        klo, khi = live_range(s, n, m, cm, free_start)
        k = np.arange(klo, khi + 1)
        neg = np.full(len(k), NEG, np.int64)
        for t in range(4):
            if t % 2 == 0:
                v = valid(np.maximum(M.get(s - op[t], klo + 1, khi + 1), Ls[t].get(s - ex[t], klo + 1, khi + 1)), k)
            else:
                v = valid(np.maximum(M.get(s - op[t], klo - 1, khi - 1), Ls[t].get(s - ex[t], klo - 1, khi - 1)) + 1, k)
            Ls[t].put(klo, v)
        c = [neg] * 3
        if sub is not None:
            c[0] = valid(M.get(s - sub, klo, khi) + 1, k)
        if ins is not None:
            c[1] = valid(M.get(s - ins, klo + 1, khi + 1), k)
        if dl is not None:
            c[2] = valid(M.get(s - dl, klo - 1, khi - 1) + 1, k)
        c += [Ls[t].get(s - ex[t], klo, khi) for t in range(4)]
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
        return -1, "", -1, -1

    # the walk
    ops = []  # from the end
    s, layer, k, i = cost, 0, end - m, end  # layer: 0 main, 1 + t for layer t
    while True:
        if layer == 0:
            if s == 0:
                assert free_start or k == 0
                ops += ["="] * (i - k)
                start = k
                break
            par = [
                (M.at(s - sub, k) + 1, 0, sub, k, "X") if sub is not None else None,
                (M.at(s - ins, k + 1), 0, ins, k + 1, "I") if ins is not None else None,
                (M.at(s - dl, k - 1) + 1, 0, dl, k - 1, "D") if dl is not None else None,
            ] + [(Ls[t].at(s - ex[t], k), 1 + t, ex[t], k, None) for t in range(4)]
            par = [q for q in par if q is not None and 0 <= q[0] <= n and 0 <= q[0] - k <= m]
            pre = max(q[0] for q in par)
            assert pre <= i
            ops += ["="] * (i - pre)
            v, layer, c, k2, o = next(q for q in par if q[0] == pre)
            if o is not None:
                ops.append(o)
            i = pre - (1 if o in ("X", "D") else 0)
            s, k = s - c, k2
        else:
            t = layer - 1
            ops.append(_LAYER_OPS[t])
            if t % 2 == 0:
                if M.at(s - op[t], k + 1) == i:
                    s, layer = s - op[t], 0
                else:
                    assert Ls[t].at(s - ex[t], k + 1) == i
                    s = s - ex[t]
                k += 1
            else:
                if M.at(s - op[t], k - 1) + 1 == i:
                    s, layer = s - op[t], 0
                else:
                    assert Ls[t].at(s - ex[t], k - 1) + 1 == i
                    s = s - ex[t]
                k, i = k - 1, i - 1
    return cost, "".join(ops[::-1]) if raw else cigar_text(ops[::-1]), start, end
