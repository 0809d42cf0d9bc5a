"""Which tiles of the tiled gap-affine traceback (pa_affine_batch_align_tiled) an alignment path crosses, from its CIGAR alone.

The geometry ("Tiled traceback"): a state (i, j), i over a and j over b, lies in row tile 0 for j = 0, else (j - 1) // 1024
(the kernel's strip of 64 lanes x 16 rows), and in column tile 0 for i = 0, else (i - 1) // tile_cols: column 0 and row 0 are border
cells of tile 0.  The walk fills one tile of codes per tile it visits, so the tile jobs of a pair are the distinct tiles of its path.
"""
from __future__ import annotations

from tests.affine_plain import cigar_elems

TILE_ROWS = 1024


def path_states(cigar: str):
    """The states (i, j) of the path, from (0, 0) to (|a|, |b|)."""
    i = j = 0
    yield (0, 0)
    for k, op in cigar_elems(cigar):
        for _ in range(k):
            if op in "=X":
                i, j = i + 1, j + 1
            elif op == "I":
                j += 1
            else:
                i += 1
            yield (i, j)


def tile_of(i: int, j: int, tile_cols: int) -> tuple[int, int]:
    """(column tile, row tile) of a state."""
    return (0 if i == 0 else (i - 1) // tile_cols, 0 if j == 0 else (j - 1) // TILE_ROWS)


def path_tiles(cigar: str, tile_cols: int) -> list[tuple[int, int]]:
    """The distinct tiles of the path, in the order it enters them from (0, 0)."""
    out = []
    for i, j in path_states(cigar):
        t = tile_of(i, j, tile_cols)
        if not out or out[-1] != t:
            assert t not in out, "a monotone path enters a tile once"
            out.append(t)
    return out


def tiles_bound(n: int, m: int, tile_cols: int) -> int:
    """No monotone path visits more tiles: one more column tile or one more row tile per move."""
    return -(-n // tile_cols) + -(-max(m, 1) // TILE_ROWS)
