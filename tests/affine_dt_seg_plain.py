"""Plain segmented traceback of the diagonal-transition route, the test oracle of AffineBatch.align_dt_seg: the fronts, recurrence,
extension and walk of tests/affine_dt_ends_plain.py, in a store that never holds more than the route claims to need.

With E the largest edge, front s is computed from fronts s - E .. s - 1, and a step of the walk lowers s by at most E.  The costs are cut
into segments of S >= E costs, segment c = [cS, cS + S - 1].

  forward   keeps a ring of the last E fronts and nothing else; a front whose cost lies in the last E of a segment (cS - E <= s < cS,
            c >= 1) is also copied to the checkpoint rows of segment c.
  rounds    from the top segment down: the store is emptied, the segment's E checkpoint rows are put at its head, the fronts
            cS .. min(cS + S - 1, cost) are computed again from them, and the walk goes on until s < cS (or ends at s = 0).

The store (`_Window`) raises on a read of a cost it does not hold, so a pass over the cases is a test of the E-rows argument: neither
the recurrence nor the walk ever looks further back.  Results are those of affine_dt_ends, plus a record of what the walk met.
"""
from __future__ import annotations

import math

import numpy as np

from tests.affine_dt_plain import NEG, gap_cost, reach
from tests.affine_plain import cigar_text, edge_costs


def max_edge(cm) -> int:
    return max(c for c in edge_costs(cm) if c is not None)


def bound_of(n: int, m: int, cm, s_max: int, free_start: bool, free_end: bool) -> int:
    """s' of the pair: min(s_max, the cost of the path that always exists)."""
    sub, ins, dl, io, ie, do, de = edge_costs(cm)
    if free_start or free_end:
        return min(s_max, gap_cost(m, ins, io, ie))
    return min(s_max, gap_cost(n, dl, do, de) + gap_cost(m, ins, io, ie))


def seg_of(bound: int, E: int, seg: int = 0) -> int:
    """The segment length of a pair whose bound is `bound`: seg, or max(E, ceil(sqrt((bound + 1) E))) for seg = 0; a length above
    max(E, bound + 1) is that (one segment)."""
    if seg == 0:
        r = math.isqrt((bound + 1) * E)
        seg = max(E, r if r * r == (bound + 1) * E else r + 1)
    assert seg >= E
    return min(seg, max(E, bound + 1))


class _Window:
    """Fronts of the three layers, by cost: only the costs put and not dropped.  A read of any other cost >= 0 raises."""

    def __init__(self):
        self.f = {}  # s -> (lo, (M, I, D))

    def put(self, s, lo, rows):
        self.f[s] = (lo, rows)

    def drop(self, s):
        self.f.pop(s, None)

    def get(self, layer, s, klo, khi):
        out = np.full(khi - klo + 1, NEG, np.int64)
        if s < 0:
            return out
        if s not in self.f:
            raise LookupError(f"front {s} is not in the store (it holds {min(self.f, default=None)} .. {max(self.f, default=None)})")
        lo, rows = self.f[s]
        arr = rows[layer]
        x0, x1 = max(klo, lo), min(khi, lo + len(arr) - 1)
        if x0 <= x1:
            out[x0 - klo:x1 - klo + 1] = arr[x0 - lo:x1 - lo + 1]
        return out

    def at(self, layer, s, k):
        return int(self.get(layer, s, k, k)[0])


def affine_dt_seg(a: bytes, b: bytes, cm, s_max: int, seg: int = 0, free_start: bool = False, free_end: bool = False):
    """-> (cost, start, end, CIGAR, record), or (-1, -1, -1, "", record) when the cost exceeds s_max.  record: "seg" the segment length
    used, "nseg" the segments of a found pair (cost // seg + 1, else 0), "crossed" the layer (0 main, 1 insert, 2 delete) the walk was
    in at every segment boundary it crossed, from the top."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8)
    B = np.frombuffer(b, np.uint8)
    sub, ins, dl, io, ie, do, de = edge_costs(cm)
    E = max_edge(cm)
    s_max = bound_of(n, m, cm, s_max, free_start, free_end)
    S = seg_of(s_max, E, seg)

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

    def step(F, s):
        """Front s from the store F: (klo, k, (M, I, D))."""
        klo = -min(m, reach(s, ins, io, ie))
        khi = n if free_start else min(n, reach(s, dl, do, de))
        k = np.arange(klo, khi + 1)
        neg = np.full(len(k), NEG, np.int64)
        Iv = Dv = neg
        if io is not None:
            Iv = valid(np.maximum(F.get(0, s - io, klo + 1, khi + 1), F.get(1, s - ie, klo + 1, khi + 1)), k)
        if do is not None:
            Dv = valid(np.maximum(F.get(0, s - do, klo - 1, khi - 1), F.get(2, s - de, klo - 1, khi - 1)) + 1, k)
        c = [neg] * 5
        if sub is not None:
            c[0] = valid(F.get(0, s - sub, klo, khi) + 1, k)
        if ins is not None:
            c[1] = valid(F.get(0, s - ins, klo + 1, khi + 1), k)
        if dl is not None:
            c[2] = valid(F.get(0, s - dl, klo - 1, khi - 1) + 1, k)
        if io is not None:
            c[3] = F.get(1, s - ie, klo, khi)
        if do is not None:
            c[4] = F.get(2, s - de, klo, khi)
        pre = np.maximum.reduce(c)
        if s == 0:
            pre = k.copy() if free_start else np.zeros(1, np.int64)
        return klo, k, (extend(pre, k), Iv, Dv)

    # the checkpoint pass: a ring of E fronts, and the last E fronts of every segment
    ring = _Window()
    ckpt = {}  # c -> {s: (lo, rows)} for cS - E <= s < cS
    cost = end = -1
    for s in range(s_max + 1):
        ring.drop(s - E - 1)
        klo, k, rows = step(ring, s)
        ring.put(s, klo, rows)
        if s % S >= S - E:
            ckpt.setdefault(s // S + 1, {})[s] = (klo, rows)
        Ms = rows[0]
        if free_end:
            hit = np.nonzero(Ms - k == m)[0]
            if len(hit):
                cost, end = s, int(Ms[hit[0]])
                break
        elif klo <= n - m <= klo + len(k) - 1 and int(Ms[n - m - klo]) == n:
            cost, end = s, n
            break
    record = {"seg": S, "nseg": 0, "crossed": []}
    if cost < 0:
        return -1, -1, -1, "", record
    del ring
    record["nseg"] = cost // S + 1

    # the rounds
    ops = []  # from the end
    s, layer, k, i = cost, 0, end - m, end
    start = None
    for c in range(cost // S, -1, -1):
        s0, s1 = c * S, min(c * S + S - 1, cost)
        F = _Window()
        for x, (lo, rows) in (ckpt.get(c, {}) if c else {}).items():
            assert s0 - E <= x < s0
            F.put(x, lo, rows)
        for x in range(s0, s1 + 1):
            lo, _, rows = step(F, x)
            F.put(x, lo, rows)
        assert s0 <= s <= s1, "the walk skipped a segment"
        while s >= s0:
            if layer == 0:
                if s == 0:
                    assert free_start or k == 0
                    ops += ["="] * (i - k)
                    start = k
                    break
                par = [
                    (F.at(0, s - sub, k) + 1, 0, sub, k, "X") if sub is not None else None,
                    (F.at(0, s - ins, k + 1), 0, ins, k + 1, "I") if ins is not None else None,
                    (F.at(0, s - dl, k - 1) + 1, 0, dl, k - 1, "D") if dl is not None else None,
                    (F.at(1, s - ie, k), 1, ie, k, None) if io is not None else None,
                    (F.at(2, s - de, k), 2, de, k, None) if do is not None else None,
                ]
                par = [q for q in par if q is not None and 0 <= q[0] <= n and 0 <= q[0] - k <= m]
                pre = max(q[0] for q in par)
                assert pre <= i
                ops += ["="] * (i - pre)
                v, layer, cst, k2, op = next(q for q in par if q[0] == pre)
                if op is not None:
                    ops.append(op)
                i = pre - (1 if op in ("X", "D") else 0)
                s, k = s - cst, k2
            elif layer == 1:
                ops.append("I")
                if F.at(0, s - io, k + 1) == i:
                    s, layer = s - io, 0
                else:
                    assert F.at(1, s - ie, k + 1) == i
                    s = s - ie
                k += 1
            else:
                ops.append("D")
                if F.at(0, s - do, k - 1) + 1 == i:
                    s, layer = s - do, 0
                else:
                    assert F.at(2, s - de, k - 1) + 1 == i
                    s = s - de
                k, i = k - 1, i - 1
        if start is not None:
            break
        record["crossed"].append(layer)
    assert start is not None and c == 0
    return cost, start, end, cigar_text(ops[::-1]), record
