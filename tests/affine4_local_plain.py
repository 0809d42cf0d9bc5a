"""Plain restatement of local (Smith-Waterman) alignment under a double-affine (two-piece) gap cost and a bonus per match, the test
oracle of pa_affine4_batch_run_local / pa_affine4_batch_align_local (include/pa_affine4_local_hip.h has the definition).

The DP runs over anti-diagonals with numpy, like affine4_plain.py, in signed scores: per cell the four layers [ins, del, ins, del]
before the main layer, with o_k, e_k the open and extend of layer k,
    L_k(i,j) = max(H(i,j-1) - (o_k + e_k), L_k(i,j-1) - e_k)    k = 0, 2
    L_k(i,j) = max(H(i-1,j) - (o_k + e_k), L_k(i-1,j) - e_k)    k = 1, 3
    H(i,j)   = max(0, H(i-1,j-1) + (match or -sub), H(i,j-1) - ins, H(i-1,j) - del, L_0, L_1, L_2, L_3)
with H = 0 and every L_k absent on row 0 and column 0.  The answer is the highest H, at the lowest i and then the lowest j; the walk
goes from there by the first parent that fits (diagonal, linear insertion, linear deletion, close of layer 0 .. 3; inside a layer open
before extend) until a main-layer state with H = 0.  The code byte is affine4_plain's with main value 7 = stop.  Gaps of different
layers, and linear against layered ones, stay separate CIGAR elements and print as I / D.
"""
from __future__ import annotations

import numpy as np

from tests.affine4_plain import _LAYER_OPS, _model, gap_cost
from tests.affine_plain import cigar_elems

NEG = -(1 << 40)  # an absent state or edge: no reachable state holds it, and it never wins against the floor at 0
STOP = 7


def local_sw4(a: bytes, b: bytes, cm, match: int, trace: bool = True):
    """-> (score, cigar, a_start, a_end, b_start, b_end); with trace=False cigar, a_start and b_start are None."""
    sub, ins, dl, op, ex = _model(cm)
    if isinstance(match, bool) or not isinstance(match, (int, np.integer)) or not 1 <= match <= 1000:
        raise ValueError("match in [1, 1000]")
    n, m = len(a), len(b)
    A = np.frombuffer(a, np.uint8).astype(np.int64)
    B = np.frombuffer(b, np.uint8).astype(np.int64)
    big = 1 << 42  # an absent edge
    sub, ins, dl = [big if c is None else int(c) for c in (sub, ins, dl)]
    H = np.zeros((n + 1, m + 1), np.int64)
    codes = np.full((n + 1, m + 1), STOP, np.uint8)
    neg = lambda: np.full(n + 1, NEG, np.int64)  # noqa: E731  a diagonal, indexed by i
    H2, H1 = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    L1 = [neg() for _ in range(4)]
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)  # cells with i >= 1 and j >= 1
        nH, nL = np.zeros(n + 1, np.int64), [neg() for _ in range(4)]
        if len(i):
            j = d - i
            eq = A[i - 1] == B[j - 1]
            lay, opened = [], []
            for k in range(4):  # insert layers come from (i, j - 1), delete layers from (i - 1, j)
                src = i if k % 2 == 0 else i - 1
                o_ = H1[src] - (op[k] + ex[k])
                lay.append(np.maximum(o_, L1[k][src] - ex[k]))
                opened.append(o_)
            cand = [H2[i - 1] + np.where(eq, match, -sub), H1[i] - ins, H1[i - 1] - dl] + lay
            h = np.maximum.reduce(cand + [np.zeros(len(i), np.int64)])
            c = np.full(len(i), 6, np.uint8)
            for k in (5, 4, 3, 2, 1, 0):
                c = np.where(h == cand[k], np.uint8(k), c)
            c = np.where(h == 0, np.uint8(STOP), c)
            for k in range(4):
                c = c | np.where(lay[k] == opened[k], 0, 8 << k).astype(np.uint8)
            H[i, j] = h
            codes[i, j] = c
            nH[i] = h
            for k in range(4):
                nL[k][i] = lay[k]
        H2, H1, L1 = H1, nH, nL
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
    layer = 0  # 0 main, 1 + k for layer k
    ops = []   # from the end: '=', 'X', 'I', 'D' (linear), _LAYER_OPS[k] inside layer k
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
    return "".join(("" if k == 1 else str(k)) + {"i": "I", "j": "I", "d": "D", "e": "D"}.get(o, o) for o, k in out), i, j


def local_verify4(cigar: str, a: bytes, b: bytes, a_start: int, b_start: int, cm, match: int):
    """Price a CIGAR on its own, from (a_start, b_start): '=' must match and scores match, 'X' must differ and scores -sub, a run of L
    'I' (adjacent I elements count as one run) scores -w_ins(L), the minimum over the linear edge and the two pieces, likewise 'D'.
    -> (score, a_end, b_end)."""
    sub, ins, dl, op, ex = _model(cm)
    i, j, score = a_start, b_start, 0
    run_op, run_len = None, 0

    def close_run():
        nonlocal score, run_op, run_len
        if run_op == "I":
            score -= gap_cost(run_len, ins, [(op[0], ex[0]), (op[2], ex[2])])
        elif run_op == "D":
            score -= gap_cost(run_len, dl, [(op[1], ex[1]), (op[3], ex[3])])
        run_op, run_len = None, 0

    for k, o in cigar_elems(cigar):
        assert k >= 1
        if o in "=X":
            close_run()
            for _ in range(k):
                assert i < len(a) and j < len(b), "CIGAR runs past a sequence"
                if o == "=":
                    assert a[i] == b[j], f"'=' on {a[i]} != {b[j]}"
                    score += match
                else:
                    assert a[i] != b[j] and sub is not None, "'X' on equal bytes or without sub"
                    score -= sub
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
    assert i <= len(a) and j <= len(b), "CIGAR runs past a sequence"
    return score, i, j
