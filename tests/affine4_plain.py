"""Plain restatements of NW::new(cm, false, false).align(a, b) over an AffineCost<4> with layers [ins, del, ins, del]
(pa-base-algos/src/nw/affine.rs, generic over the number of layers), the test oracles of the batched double-affine kernel.

Three things that share as little as they can:
  * affine4_nw: the layered DP over anti-diagonals with numpy, like tests/affine_plain.py.  Per cell the layers come in index order before
    the main layer (EditGraph::iterate_layers, edit_graph.rs:82-87); every state takes the minimum over the parents of
    EditGraph::iterate_parents (edit_graph.rs:96-169), capped at INF, and records its FIRST parent in that order whose cost fits.  The
    walk from (n, m, main) to (0, 0, main) follows those records.  Ops of different layers, and linear against affine ones, stay separate
    elements (AffineCigar::push_op merges equal ops only) before they print as I / D.
  * general_gap_cost: a general-gap DP without layers, M(i,j) = min(diagonal, min_L M(i,j-L) + w_ins(L), min_L M(i-L,j) + w_del(L)),
    where w(L) is the minimum over the linear edge and the two pieces.  O(n^2 m): for pairs up to about 60 bytes.
  * affine4_verify: prices a CIGAR on its own, a run of L gaps by w(L), and checks that it consumes both sequences.
"""
from __future__ import annotations

import numpy as np

from tests.affine_plain import cigar_elems

INF = 1 << 30
KINDS = ["ins", "del", "ins", "del"]


def _model(cm):
    if [k for k, _, _ in cm.layers] != KINDS:
        raise ValueError("layers [ins, del, ins, del] only")
    return cm.sub, cm.ins, cm.del_, [int(o) for _, o, _ in cm.layers], [int(e) for _, _, e in cm.layers]


def affine4_nw(a: bytes, b: bytes, cm, trace: bool = True, raw: bool = False):
    """-> (cost, CIGAR or None); with raw the walk's ops before printing, one character a step ('=', 'X', linear 'I' / 'D', and
    _LAYER_OPS for a step inside layer 0 .. 3), in place of the CIGAR."""
    sub, ins, dl, op, ex = _model(cm)
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8).astype(np.int64)
    B = np.frombuffer(b, np.uint8).astype(np.int64)
    big = 4 * INF  # an absent edge: never below INF
    sub, ins, dl = [big if c is None else int(c) for c in (sub, ins, dl)]
    codes = np.zeros((n + 1, m + 1), np.uint8) if trace else None
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
        # main layer, in iterate_parents order: match / substitution, ins, del, close of layer 0 .. 3
        cand = [np.where(dg, Mdiag + np.where(eq, 0, sub), big), Mup + ins, Mleft + dl] + lay
        M = np.minimum.reduce(cand + [np.full(len(i), INF, np.int64)])
        if d == 0:
            M[:] = 0
        if trace:
            c = np.full(len(i), 6, np.uint8)
            for k in (5, 4, 3, 2, 1, 0):
                c = np.where(M == cand[k], np.uint8(k), c)
            for k in range(4):
                c = c | np.where(lay[k] == opened[k], 0, 8 << k).astype(np.uint8)
            codes[i, j] = c
        nM = full()
        nM[i] = M
        nL = [full() for _ in range(4)]
        for k in range(4):
            nL[k][i] = lay[k]
        M2, M1, L1 = M1, nM, nL
    cost = int(M1[n])
    if not trace:
        return cost, None
    return cost, _walk(a, b, codes, raw)


_LAYER_OPS = "idje"  # a step inside layer 0 .. 3: distinct ops, so that only gaps of one layer merge


def _walk(a, b, codes, raw=False) -> str:
    i, j, layer = len(a), len(b), 0  # layer: 0 main, 1 + k for layer k
    ops = []
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
    if raw:
        return "".join(ops[::-1])
    out = []
    for op in ops[::-1]:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return "".join(("" if k == 1 else str(k)) + {"i": "I", "j": "I", "d": "D", "e": "D"}.get(op, op) for op, k in out)


def gap_cost(L: int, lin, pieces) -> int:
    """w(L): the cheapest way to pay one gap of length L, over the linear edge (None: absent) and the (open, extend) pieces."""
    opts = [o + L * e for o, e in pieces] + ([L * lin] if lin is not None else [])
    return min(opts)


def general_gap_cost(a: bytes, b: bytes, cm) -> int:
    """The cost by a DP that has no layers: a gap of any length is one edge priced by w(L).  Shares nothing with affine4_nw."""
    sub, ins, dl, op, ex = _model(cm)
    n, m = len(a), len(b)
    wi = [0] + [gap_cost(L, ins, [(op[0], ex[0]), (op[2], ex[2])]) for L in range(1, m + 1)]
    wd = [0] + [gap_cost(L, dl, [(op[1], ex[1]), (op[3], ex[3])]) for L in range(1, n + 1)]
    M = [[INF] * (m + 1) for _ in range(n + 1)]
    M[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            best = INF
            if i and j:
                if a[i - 1] == b[j - 1]:
                    best = M[i - 1][j - 1]
                elif sub is not None:
                    best = M[i - 1][j - 1] + sub
            for L in range(1, j + 1):
                best = min(best, M[i][j - L] + wi[L])
            for L in range(1, i + 1):
                best = min(best, M[i - L][j] + wd[L])
            M[i][j] = best
    return M[n][m]


def affine4_verify(cigar: str, a: bytes, b: bytes, cm) -> int:
    """Price a CIGAR on its own: '=' must match and costs 0, 'X' must differ and costs sub, a run of L 'I' (adjacent I elements
    count as one run) costs w_ins(L), likewise 'D'.  The CIGAR must consume a and b exactly."""
    sub, ins, dl, op, ex = _model(cm)
    i = j = cost = 0
    run_op, run_len = None, 0

    def close_run():
        nonlocal cost, run_op, run_len
        if run_op == "I":
            cost += gap_cost(run_len, ins, [(op[0], ex[0]), (op[2], ex[2])])
        elif run_op == "D":
            cost += gap_cost(run_len, dl, [(op[1], ex[1]), (op[3], ex[3])])
        run_op, run_len = None, 0

    for k, o in cigar_elems(cigar):
        assert k >= 1
        if o in "=X":
            close_run()
            for _ in range(k):
                assert i < len(a) and j < len(b), "CIGAR runs past a sequence"
                if o == "=":
                    assert a[i] == b[j], f"'=' on {a[i]} != {b[j]}"
                else:
                    assert a[i] != b[j] and sub is not None, "'X' on equal bytes or without sub"
                    cost += sub
                i, j = i + 1, j + 1
        else:
            if run_op != o:
                close_run()
            run_op, run_len = o, run_len + k
            if o == "I":
                j += k
            else:
                i += k
    close_run()
    assert (i, j) == (len(a), len(b)), f"CIGAR consumes ({i}, {j}) of ({len(a)}, {len(b)})"
    return cost
