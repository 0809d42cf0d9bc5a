"""Plain segmented traceback of the double-affine diagonal-transition route, the test oracle of Affine4Batch.align_dt_segmented: the
fronts, recurrence, extension and walk of tests/affine4_dt_plain.py, in a store that never holds more than the route claims to need.
tests/affine_dt_seg_plain.py restated for five rings with depths of their own.

With E the largest of sub, ins, del (those present) and open_0 .. open_3, and e_t = extend_t: front s reads the main layer at
s - {sub, ins, del, open_t} >= s - E and layer t at s - e_t only, and the walk reads the same fronts.  One walk step lowers s by at most
Ew = max(E, e_0 .. e_3), which can exceed E.  The costs are cut into segments of S >= Ew costs, segment c = [cS, cS + S - 1].  Ring 0 is
the main layer and keeps h_0 = E fronts below a segment, ring 1 + t is layer t and keeps h_{1+t} = e_t: H = E + e_0 + e_1 + e_2 + e_3
rows in all, not 5 Ew.

  forward   keeps the last E fronts of the main layer and the last e_t of layer t and nothing else; the front of ring r whose cost lies
            in the last h_r of a segment (cS - h_r <= s < cS, c >= 1) is also copied to the checkpoint rows of segment c.
  rounds    from the top segment down: the stores are emptied, the segment's checkpoint rows are put at the head of each ring, the
            fronts cS .. min(cS + S - 1, cost) are computed again from them, and the walk goes on until s < cS (or ends at s = 0).

The store is per ring (`_Ring`) and raises on a read of a cost it does not hold, so a pass over the cases is a test of the argument:
neither the recurrence nor the walk ever looks further back than h_r in ring r.  Results are those of affine4_dt, plus a record of what
the walk met.
"""
from __future__ import annotations

import math

import numpy as np

from tests.affine4_dt_plain import bound_of, cigar_text, live_range  # noqa: F401
from tests.affine4_plain import _LAYER_OPS, _model
from tests.affine_dt_plain import NEG


def heads(cm):
    """(h_0 .. h_4): the fronts ring r keeps below a segment."""
    sub, ins, dl, op, ex = _model(cm)
    return (max([c for c in (sub, ins, dl) if c is not None] + list(op)),) + tuple(ex)


def E_of(cm) -> int:
    return heads(cm)[0]


def H(cm) -> int:
    return sum(heads(cm))


def Ew(cm) -> int:
    return max(heads(cm))


def seg_of(bound: int, cm, seg: int = 0, unchecked: bool = False) -> int:
    """The segment length of a pair whose bound is `bound`: seg, or for seg = 0 the smallest S with 5 S^2 >= (bound + 1) H raised to
    Ew; a length above max(Ew, bound + 1) is that (one segment).  unchecked: `seg` as it is, even below Ew (the tests of the argument)."""
    if unchecked:
        return seg
    if seg == 0:
        x = -(-(bound + 1) * H(cm) // 5)
        r = math.isqrt(x)
        seg = max(Ew(cm), r if r * r == x else r + 1)
    assert seg >= Ew(cm)
    return min(seg, max(Ew(cm), bound + 1))


class _Ring:
    """Fronts of one ring, by cost: only the costs put and not dropped.  A read of any other cost >= 0 raises."""

    def __init__(self, name=""):
        self.name = name
        self.f = {}  # s -> (lo, array)

    def put(self, s, lo, arr):
        self.f[s] = (lo, arr)

    def drop(self, s):
        self.f.pop(s, None)

    def get(self, s, klo, khi):
        out = np.full(khi - klo + 1, NEG, np.int64)
        if s < 0:
            return out
        if s not in self.f:
            raise LookupError(f"front {s} is not in ring {self.name} (it holds {min(self.f, default=None)} .. {max(self.f, default=None)})")
        lo, arr = self.f[s]
        x0, x1 = max(klo, lo), min(khi, lo + len(arr) - 1)
        if x0 <= x1:
            out[x0 - klo:x1 - klo + 1] = arr[x0 - lo:x1 - lo + 1]
        return out

    def at(self, s, k):
        return int(self.get(s, k, k)[0])


def affine4_dt_seg(a: bytes, b: bytes, cm, s_max: int, seg: int = 0, free_start: bool = False, free_end: bool = False, unchecked: bool = False):
    """-> (cost, start, end, CIGAR, record), or (-1, -1, -1, "", record) when the cost exceeds s_max.  record: "seg" the segment length
    used, "nseg" the segments of a found pair (cost // seg + 1, else 0), "crossed" the layer (0 main, 1 + t inside layer t) the walk
    was in at every segment boundary it crossed, from the top.  unchecked: run with S = seg even where seg < Ew, which the route
    refuses: the stores then raise, or the walk skips a segment."""
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8)
    B = np.frombuffer(b, np.uint8)
    sub, ins, dl, op, ex = _model(cm)
    h = heads(cm)
    s_max = bound_of(n, m, cm, s_max, free_start, free_end)
    S = seg_of(s_max, cm, seg, unchecked)

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

    def step(R, s):
        """Front s from the rings R: (klo, k, [M, L_0 .. L_3])."""
        klo, khi = live_range(s, n, m, cm, free_start)
        k = np.arange(klo, khi + 1)
        neg = np.full(len(k), NEG, np.int64)
        Ls = []
        for t in range(4):
            if t % 2 == 0:
                Ls.append(valid(np.maximum(R[0].get(s - op[t], klo + 1, khi + 1), R[1 + t].get(s - ex[t], klo + 1, khi + 1)), k))
            else:
                Ls.append(valid(np.maximum(R[0].get(s - op[t], klo - 1, khi - 1), R[1 + t].get(s - ex[t], klo - 1, khi - 1)) + 1, k))
        c = [neg] * 3
        if sub is not None:
            c[0] = valid(R[0].get(s - sub, klo, khi) + 1, k)
        if ins is not None:
            c[1] = valid(R[0].get(s - ins, klo + 1, khi + 1), k)
        if dl is not None:
            c[2] = valid(R[0].get(s - dl, klo - 1, khi - 1) + 1, k)
        c += [R[1 + t].get(s - ex[t], klo, khi) for t in range(4)]
        pre = np.maximum.reduce(c)
        if s == 0:
            pre = k.copy() if free_start else np.zeros(1, np.int64)
        return klo, k, [extend(pre, k)] + Ls

    # the checkpoint pass: per ring the last h_r fronts, and the last h_r fronts of every segment
    ring = [_Ring(str(r)) for r in range(5)]
    ckpt = {}  # c -> [{s: (lo, array)} per ring] for cS - h_r <= s < cS
    cost = end = -1
    for s in range(s_max + 1):
        for r in range(5):
            ring[r].drop(s - h[r] - 1)
        klo, k, rows = step(ring, s)
        for r in range(5):
            ring[r].put(s, klo, rows[r])
            if s % S >= S - h[r]:
                ckpt.setdefault(s // S + 1, [{} for _ in range(5)])[r][s] = (klo, rows[r])
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
        F = [_Ring(str(r)) for r in range(5)]
        if c:
            for r in range(5):
                for x, (lo, arr) in ckpt[c][r].items():
                    assert s0 - h[r] <= x < s0
                    F[r].put(x, lo, arr)
        for x in range(s0, s1 + 1):
            lo, _, rows = step(F, x)
            for r in range(5):
                F[r].put(x, lo, rows[r])
        assert s0 <= s <= s1, "the walk skipped a segment"
        while s >= s0:
            if layer == 0:
                if s == 0:
                    assert free_start or k == 0
                    ops += ["="] * (i - k)
                    start = k
                    break
                par = [
                    (F[0].at(s - sub, k) + 1, 0, sub, k, "X") if sub is not None else None,
                    (F[0].at(s - ins, k + 1), 0, ins, k + 1, "I") if ins is not None else None,
                    (F[0].at(s - dl, k - 1) + 1, 0, dl, k - 1, "D") if dl is not None else None,
                ] + [(F[1 + t].at(s - ex[t], k), 1 + t, ex[t], k, None) for t in range(4)]
                par = [q for q in par if q is not None and 0 <= q[0] <= n and 0 <= q[0] - k <= m]
                pre = max(q[0] for q in par)
                assert pre <= i
                ops += ["="] * (i - pre)
                v, layer, cst, k2, o = next(q for q in par if q[0] == pre)
                if o is not None:
                    ops.append(o)
                i = pre - (1 if o in ("X", "D") else 0)
                s, k = s - cst, k2
            else:
                t = layer - 1
                ops.append(_LAYER_OPS[t])
                if t % 2 == 0:
                    if F[0].at(s - op[t], k + 1) == i:
                        s, layer = s - op[t], 0
                    else:
                        assert F[1 + t].at(s - ex[t], k + 1) == i
                        s = s - ex[t]
                    k += 1
                else:
                    if F[0].at(s - op[t], k - 1) + 1 == i:
                        s, layer = s - op[t], 0
                    else:
                        assert F[1 + t].at(s - ex[t], k - 1) + 1 == i
                        s = s - ex[t]
                    k, i = k - 1, i - 1
        if start is not None:
            break
        record["crossed"].append(layer)
    assert start is not None and c == 0
    return cost, start, end, cigar_text(ops[::-1]), record
