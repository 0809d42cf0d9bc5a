"""CPU-side checks of the tiled gap-affine traceback: the header's declarations, the exported symbols, the C ABI's argument check that
runs before any device is touched, and the path-to-tiles helper of the GPU tests on hand-worked paths."""
import re
from pathlib import Path

from astar_pairwise_aligner_amd import capi
from tests import affine_tiles_plain as tiles

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4


def test_header_declares_the_tiled_api():
    txt = (ROOT / "include" / "pa_affine_hip.h").read_text()
    for fn in ("pa_affine_batch_align_tiled", "pa_affine_batch_tiled_info"):
        assert re.search(r"\b" + fn + r"\(", txt), fn
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn)
    assert re.search(r"int pa_affine_batch_align_tiled\(pa_affine_batch\* ab, uint32_t tile_cols,\s*int32_t\* cost_out, char\*\* cigar_out,"
                     r"\s*float\* forward_ms,\s*float\* refill_ms, float\* walk_ms\);", txt)


def test_null_batch_is_an_argument_error():
    L = capi.load()
    assert L.pa_affine_batch_align_tiled(None, 0, None, None, None, None, None) == PA_E_ARG
    assert capi.last_error().startswith("pa_affine_batch_align_tiled:")
    L.pa_affine_batch_tiled_info(None, None, None, None, None, None)  # a NULL batch and NULL outputs are accepted


def test_tile_of_a_state():
    assert tiles.tile_of(0, 0, 64) == (0, 0)
    assert tiles.tile_of(64, 1024, 64) == (0, 0)  # the last column and the last row of tile (0, 0)
    assert tiles.tile_of(65, 1024, 64) == (1, 0)
    assert tiles.tile_of(64, 1025, 64) == (0, 1)
    assert tiles.tile_of(0, 3000, 64) == (0, 2) and tiles.tile_of(3000, 0, 1024) == (2, 0)


def test_hand_worked_paths():
    # the diagonal of two identical sequences of 2048 at 1024 columns: (1024, 1024) is the corner of tile (0, 0), (1025, 1025) the
    # first state of tile (1, 1) -- the path crosses the corner and never enters (0, 1) or (1, 0)
    assert tiles.path_tiles("2048=", 1024) == [(0, 0), (1, 1)]
    # the same with one deletion after the corner: (1025, 1024) is in column tile 1 and still in row tile 0
    assert tiles.path_tiles("1024=D1023=", 1024) == [(0, 0), (1, 0), (1, 1)]
    # column 0 through three strips; row 0 through three column tiles
    assert tiles.path_tiles("3000I", 64) == [(0, 0), (0, 1), (0, 2)]
    assert tiles.path_tiles("130D", 64) == [(0, 0), (1, 0), (2, 0)]
    # 100 matches end in column 100 (column tile 1 of 64), 30 insertions stay there, 100 more matches reach column 200 (tile 3)
    assert tiles.path_tiles("100=30I100=", 64) == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert tiles.path_tiles("", 64) == [(0, 0)]
    assert list(tiles.path_states("=XID")) == [(0, 0), (1, 1), (2, 2), (2, 3), (3, 3)]


def test_bound_on_the_tiles_of_a_path():
    assert tiles.tiles_bound(2048, 2048, 1024) == 4
    assert tiles.tiles_bound(0, 3000, 64) == 3 and tiles.tiles_bound(130, 0, 64) == 4
    assert tiles.tiles_bound(0, 0, 64) == 1
    for cigar, n, m, c in (("2048=", 2048, 2048, 1024), ("3000I", 0, 3000, 64), ("130D", 130, 0, 64), ("100=30I100=", 200, 230, 64)):
        assert len(tiles.path_tiles(cigar, c)) <= tiles.tiles_bound(n, m, c)
