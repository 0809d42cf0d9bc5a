"""A plain restatement of the tiled double-affine traceback (pa_affine4_batch_align_tiled, csrc/affine4_tile_kernel.hpp), cell by cell.

Three steps, as on the device, with the tile height `tile_rows` (the kernel's strip of 64 x 16 rows) and the tile width `tile_cols` as
arguments, so that a test can run the whole scheme on pairs of a few dozen bytes:
  * checkpoint_pass: the cost-only DP, column by column, which keeps nothing but
      - the row checkpoints: (M, I1, I2) of every column of the last row of every row tile but the last;
      - the column checkpoints: (M, D1, D2) of every row, row 0 included, after columns C, 2C, .. < |a|.
  * fill_tile: the traceback codes of one tile from the checkpoints to its left and above it (row 0 of row tile 0 restarted from its
    own checkpoint), only up to the walk's state.
  * walk_tile: the reference's backward walk from a stored state (i, j, layer) until it leaves the tile or reaches (0, 0, main).
Everything the fill and the walk read goes through a Store that raises on any read outside the checkpoints and the current tile, so a
scheme that needed a value it does not keep cannot pass by accident.

Geometry: state (i, j) lies in row tile 0 for j = 0, else (j - 1) // tile_rows, and in column tile 0 for i = 0, else (i - 1) //
tile_cols.  Codes and walk are those of tests/affine4_plain.py (first parent in iterate_parents order; layer ops kept apart).
"""
from __future__ import annotations

from tests.affine4_plain import INF, _LAYER_OPS, _model

BIG = 4 * INF  # an absent edge: never below INF


class Store:
    """The checkpoints of one pair and the codes of the one tile that is filled at the moment."""

    def __init__(self):
        self.rows = {}   # (row tile s, column i) -> (M, I1, I2) of row (s + 1) tile_rows
        self.cols = {}   # (checkpoint k, row j) -> (M, D1, D2) of column (k + 1) tile_cols
        self.tile = {}   # (i, j) -> code, of the current tile only
        self.reads = 0

    def row(self, s, i):
        self.reads += 1
        return self.rows[(s, i)]  # KeyError: not a checkpoint

    def col(self, k, j):
        self.reads += 1
        return self.cols[(k, j)]

    def code(self, i, j):
        return self.tile[(i, j)]  # KeyError: outside the current tile, or beyond what the fill computed

    def values(self):
        return len(self.rows) + len(self.cols)


def _costs(cm):
    sub, ins, dl, op, ex = _model(cm)
    sub, ins, dl = [BIG if c is None else int(c) for c in (sub, ins, dl)]
    return sub, ins, dl, [o + e for o, e in zip(op, ex)], ex


def _row0(c, M, D1, D2, origin):
    """Row 0 of one column from row 0 of the column before it: (M, D1, D2, code)."""
    sub, ins, dl, oe, e = c
    d1o, d2o, cdl = M + oe[1], M + oe[3], M + dl
    nD1, nD2 = min(d1o, D1 + e[1], INF), min(d2o, D2 + e[3], INF)
    nM = 0 if origin else min(cdl, nD1, nD2, INF)
    code = (2 if nM == cdl else 4 if nM == nD1 else 6) | (0 if nD1 == d1o else 16) | (0 if nD2 == d2o else 64)
    return nM, nD1, nD2, code


def _cell(c, eq, Mdiag, up, left):
    """One cell below row 0: up = (M, I1, I2) of the row above in this column, left = (M, D1, D2) of this row in the column before.
    -> (M, I1, I2, D1, D2, code)."""
    sub, ins, dl, oe, e = c
    Mup, I1up, I2up = up
    Ml, D1l, D2l = left
    i1o, i2o, d1o, d2o = Mup + oe[0], Mup + oe[2], Ml + oe[1], Ml + oe[3]
    I1, I2 = min(i1o, I1up + e[0], INF), min(i2o, I2up + e[2], INF)
    D1, D2 = min(d1o, D1l + e[1], INF), min(d2o, D2l + e[3], INF)
    cand = [Mdiag + (0 if eq else sub), Mup + ins, Ml + dl, I1, D1, I2, D2]
    M = min(cand + [INF])
    code = next((k for k in range(7) if cand[k] == M), 6)
    code |= (0 if I1 == i1o else 8) | (0 if D1 == d1o else 16) | (0 if I2 == i2o else 32) | (0 if D2 == d2o else 64)
    return M, I1, I2, D1, D2, code


def row_tiles(m, tile_rows):
    return max(1, -(-m // tile_rows))


def checkpoint_pass(a: bytes, b: bytes, cm, tile_rows: int, tile_cols: int):
    """-> (cost, Store).  Two columns of state at a time; nothing else is kept but the checkpoints."""
    c = _costs(cm)
    n, m = len(a), len(b)
    S = row_tiles(m, tile_rows)
    st = Store()
    prev = [(INF, INF, INF)] * (m + 1)  # (M, D1, D2) of the column before, by row
    r0 = (INF, INF, INF)
    for i in range(n + 1):
        M0, D10, D20, _ = _row0(c, *r0, i == 0)
        r0 = (M0, D10, D20)
        cur = [r0]
        up = (M0, INF, INF)
        Mdiag = prev[0][0]
        for j in range(1, m + 1):
            M, I1, I2, D1, D2, _ = _cell(c, i > 0 and a[i - 1] == b[j - 1], Mdiag if i > 0 else INF, up, prev[j])
            Mdiag = prev[j][0]
            cur.append((M, D1, D2))
            up = (M, I1, I2)
            if j % tile_rows == 0 and j // tile_rows < S:
                st.rows[(j // tile_rows - 1, i)] = up
        if i > 0 and i % tile_cols == 0 and i < n:
            for j in range(m + 1):
                st.cols[(i // tile_cols - 1, j)] = cur[j]
        prev = cur
    return prev[m][0], st


def tile_of(i, j, tile_rows, tile_cols):
    """(column tile, row tile) of a state."""
    return (0 if i == 0 else (i - 1) // tile_cols, 0 if j == 0 else (j - 1) // tile_rows)


def fill_tile(st: Store, a: bytes, b: bytes, cm, tile_rows: int, tile_cols: int, i1: int, j1: int):
    """The codes of the tile of state (i1, j1), columns up to i1 and rows up to j1, into st.tile (which it replaces)."""
    c = _costs(cm)
    ct, rt = tile_of(i1, j1, tile_rows, tile_cols)
    c0, jt = ct * tile_cols, rt * tile_rows
    cs = c0 + 1 if c0 else 0
    st.tile = {}
    # the column left of the tile, rows jt + 1 .. j1, and M of row jt there (the first diagonal)
    if c0:
        left = {j: st.col(ct - 1, j) for j in range(jt + 1, j1 + 1)}
        r0 = st.col(ct - 1, 0) if rt == 0 else None
        Mcorner = r0[0] if rt == 0 else st.row(rt - 1, c0)[0]
    else:
        left = {j: (INF, INF, INF) for j in range(jt + 1, j1 + 1)}
        r0 = (INF, INF, INF)
        Mcorner = INF
    for i in range(cs, i1 + 1):
        if rt == 0:
            M0, D10, D20, code = _row0(c, *r0, i == 0)
            r0 = (M0, D10, D20)
            st.tile[(i, 0)] = code
            up = (M0, INF, INF)
        else:
            up = st.row(rt - 1, i)
        Mdiag, Mcorner = Mcorner, up[0]
        for j in range(jt + 1, j1 + 1):
            M, I1, I2, D1, D2, code = _cell(c, i > 0 and a[i - 1] == b[j - 1], Mdiag if i > 0 else INF, up, left[j])
            Mdiag = left[j][0]
            left[j] = (M, D1, D2)
            up = (M, I1, I2)
            st.tile[(i, j)] = code


def walk_tile(st: Store, a: bytes, b: bytes, tile_rows: int, tile_cols: int, state, ops: list):
    """From `state` = (i, j, layer) through the codes of its tile; appends the ops (from the end backwards) and returns the state at
    which the walk left the tile or reached (0, 0, main)."""
    i, j, layer = state
    home = tile_of(i, j, tile_rows, tile_cols)
    while (i, j, layer) != (0, 0, 0) and tile_of(i, j, tile_rows, tile_cols) == home:
        code = st.code(i, j)
        if layer == 0:
            k = code & 7
            if k == 0:
                assert i > 0 and j > 0
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
            if not code & (8 << k):
                layer = 0
        assert i >= 0 and j >= 0
    return i, j, layer


def cigar_of(ops) -> str:
    out = []
    for op in ops[::-1]:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return "".join(("" if k == 1 else str(k)) + {"i": "I", "j": "I", "d": "D", "e": "D"}.get(op, op) for op, k in out)


def tiles_bound(n, m, tile_rows, tile_cols):
    """No monotone path visits more tiles: one more column tile or one more row tile per move."""
    return -(-n // tile_cols) + -(-max(m, 1) // tile_rows)


def affine4_tiled(a: bytes, b: bytes, cm, tile_rows: int, tile_cols: int):
    """-> (cost, CIGAR, [(tile, state at entry)] in walk order, Store)."""
    cost, st = checkpoint_pass(a, b, cm, tile_rows, tile_cols)
    state = (len(a), len(b), 0)
    ops, visited = [], []
    while state != (0, 0, 0):
        assert len(visited) < tiles_bound(len(a), len(b), tile_rows, tile_cols), "the rounds must end"
        visited.append((tile_of(state[0], state[1], tile_rows, tile_cols), state))
        fill_tile(st, a, b, cm, tile_rows, tile_cols, state[0], state[1])
        state = walk_tile(st, a, b, tile_rows, tile_cols, state, ops)
    return cost, cigar_of(ops), visited, st
