"""Plain restatement of NW::new(cm, false, false).align(a, b) over AffineCost<0> / AffineCost<2> (pa-base-algos/src/nw/affine.rs), the
test oracle of the batched gap-affine kernel.

The DP runs over anti-diagonals with numpy.  Per cell, the affine layers come before the main layer (EditGraph::iterate_layers,
edit_graph.rs:82-87) and every state takes the minimum over the parents of EditGraph::iterate_parents (edit_graph.rs:96-169), capped at
INF like AffineNwFront (nw/affine.rs:13, 84-106, 133-162).  For the traceback every cell also records its FIRST parent in
iterate_parents order whose cost fits (AffineNwFronts::parent, nw/affine.rs:164-188), and the walk from (n, m, main) to (0, 0, main)
follows those records (trace, :283-305).  The CIGAR keeps linear and affine gaps as separate elements before printing them as I / D,
like AffineCigar::to_base (pa-affine-types/src/cigar.rs:111-124), so a path that put a linear and an affine gap side by side would show
as two adjacent elements of the same letter.
"""
from __future__ import annotations

import re

import numpy as np

INF = 1 << 30


def edge_costs(cm):
    """(sub, ins, del, ins_open, ins_extend, del_open, del_extend) of an AffineCost, None for a missing edge."""
    il, dl = cm.ins_layer(), cm.del_layer()
    return (cm.sub, cm.ins, cm.del_, il and il[0], il and il[1], dl and dl[0], dl and dl[1])


def affine_nw(a: bytes, b: bytes, cm, trace: bool = True, raw: bool = False):
    """-> (cost, CIGAR or None); with raw the walk's ops before printing, one character a step ('=', 'X', linear 'I' / 'D', affine
    'i' / 'd'), in place of the CIGAR."""
    if len(cm.layers) > 2 or [k for k, _, _ in cm.layers] not in ([], ["ins", "del"]):
        raise ValueError("N in {0, 2} only")
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8).astype(np.int64)
    B = np.frombuffer(b, np.uint8).astype(np.int64)
    big = 4 * INF  # an absent edge: never below INF
    sub, ins, dl, io, ie, do, de = [big if c is None else int(c) for c in edge_costs(cm)]
    codes = np.zeros((n + 1, m + 1), np.uint8) if trace else None
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
        # insert layer: open from M(i, j-1), extend from I(i, j-1); delete layer: from (i-1, j)
        iop, iex = Mup + io, Iup + ie
        I = np.minimum(np.minimum(iop, iex), INF)
        dop, dex = Mleft + do, Dleft + de
        D = np.minimum(np.minimum(dop, dex), INF)
        # main layer, in iterate_parents order: match / substitution, ins, del, close insert layer, close delete layer
        cand = [np.where(dg, Mdiag + np.where(eq, 0, sub), big), Mup + ins, Mleft + dl, I + ie, D + de]
        M = np.minimum.reduce(cand + [np.full(len(i), INF, np.int64)])
        if d == 0:
            M[:] = 0
        if trace:
            c = np.full(len(i), 4, np.uint8)
            for k in (3, 2, 1, 0):
                c = np.where(M == cand[k], np.uint8(k), c)
            c = c | np.where(I == iop, 0, 8).astype(np.uint8) | np.where(D == dop, 0, 16).astype(np.uint8)
            codes[i, j] = c
        nM, nI, nD = full(), full(), full()
        nM[i], nI[i], nD[i] = M, I, D
        M2, M1, I1, D1 = M1, nM, nI, nD
    cost = int(M1[n])
    if not trace:
        return cost, None
    return cost, _walk(a, b, codes, raw)


def _walk(a, b, codes, raw=False) -> str:
    i, j, layer = len(a), len(b), 0
    ops = []  # from the end: '=', 'X', 'I', 'D' (linear), 'i', 'd' (affine)
    while (i, j, layer) != (0, 0, 0):
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
    if raw:
        return "".join(ops[::-1])
    return cigar_text(ops[::-1])


def cigar_text(ops) -> str:
    """Run-length text of a list of ops: same ops merge (AffineCigar::push_op), affine ones print as I / D, count 1 left out."""
    out = []
    for op in ops:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return "".join(("" if k == 1 else str(k)) + op.upper() for op, k in out)


_ELEM = re.compile(r"(\d*)([=XID])")


def cigar_elems(cigar: str):
    pos, out = 0, []
    for mt in _ELEM.finditer(cigar):
        assert mt.start() == pos, f"bad CIGAR {cigar!r}"
        pos = mt.end()
        out.append((int(mt.group(1) or 1), mt.group(2)))
    assert pos == len(cigar), f"bad CIGAR {cigar!r}"
    return out


def affine_verify(cigar: str, a: bytes, b: bytes, cm) -> int:
    """Price a CIGAR on its own: '=' must match and costs 0, 'X' must differ and costs sub, a run of L 'I' costs min(L ins,
    open + L extend) over the edges that exist, likewise 'D'.  The CIGAR must consume a and b exactly."""
    sub, ins, dl, io, ie, do, de = edge_costs(cm)
    i = j = cost = 0
    for k, op in cigar_elems(cigar):
        assert k >= 1
        if op in "=X":
            for _ in range(k):
                assert i < len(a) and j < len(b), "CIGAR runs past a sequence"
                if op == "=":
                    assert a[i] == b[j], f"'=' on {a[i]} != {b[j]}"
                else:
                    assert a[i] != b[j] and sub is not None, "'X' on equal bytes or without sub"
                    cost += sub
                i, j = i + 1, j + 1
        else:
            lin, op_, ex = (ins, io, ie) if op == "I" else (dl, do, de)
            opts = ([k * lin] if lin is not None else []) + ([op_ + k * ex] if op_ is not None else [])
            assert opts, f"no edge for {op}"
            cost += min(opts)
            if op == "I":
                j += k
            else:
                i += k
    assert (i, j) == (len(a), len(b)), f"CIGAR consumes ({i}, {j}) of ({len(a)}, {len(b)})"
    return cost


def no_adjacent_same_op(cigar: str) -> bool:
    ops = [op for _, op in cigar_elems(cigar)]
    return all(x != y for x, y in zip(ops, ops[1:]))
