"""CPU-side checks of the tiled double-affine API: the header of its own and what capi binds, the binding's argument checks (they come
before the library is called), the C ABI's NULL handling, and the loud failure without a GPU."""
import ctypes as C
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
FUNCS = ("pa_affine4_batch_align_tiled", "pa_affine4_batch_tiled_info")
DOUBLE = AffineCost.double_affine(4, 6, 2, 24, 1)
PA_E_ARG = -4


def test_header_declares_exactly_what_capi_binds():
    txt = (ROOT / "include" / "pa_affine4_tiled_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert set(re.findall(r"\b(pa_[a-z_0-9]+)\s*\(", code)) == set(FUNCS)
    assert re.search(r"int pa_affine4_batch_align_tiled\(pa_affine4_batch\* ab, uint32_t tile_cols,\s*int32_t\* cost_out, char\*\* cigar_out,"
                     r"\s*float\* forward_ms,\s*float\* refill_ms, float\* walk_ms\);", code)
    assert re.search(r"void pa_affine4_batch_tiled_info\(const pa_affine4_batch\* ab, double\* chunks, double\* rounds, double\* tile_jobs,"
                     r"\s*double\* refill_cells,\s*double\* chunk_bytes_max\);", code)
    assert '#include "pa_affine4_hip.h"' in code
    L = capi.load()
    for fn in FUNCS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(L, fn)
    assert L.pa_affine4_batch_align_tiled.argtypes[1] is C.c_uint32 and len(L.pa_affine4_batch_align_tiled.argtypes) == 7
    assert len(L.pa_affine4_batch_tiled_info.argtypes) == 6 and L.pa_affine4_batch_tiled_info.restype is None
    # the byte formula is stated where the functions are declared, and the untiled header points here
    for word in ("(strips - 1) * (|a| + 1) * 16", "(H + 1) * 12", "(min(|a|, C) + 1) * (min(H, 64 R) + 1)", "|a| + |b|"):
        assert word in txt, word
    assert "pa_affine4_tiled_hip.h" in (ROOT / "include" / "pa_affine4_hip.h").read_text()


def test_null_batch_is_an_argument_error():
    L = capi.load()
    assert L.pa_affine4_batch_align_tiled(None, 0, None, None, None, None, None) == PA_E_ARG
    assert capi.last_error().startswith("pa_affine4_batch_align_tiled:")
    L.pa_affine4_batch_tiled_info(None, None, None, None, None, None)  # a NULL batch and NULL outputs are accepted
    vals = [C.c_double(7) for _ in range(5)]
    L.pa_affine4_batch_tiled_info(None, *[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0] * 5


@pytest.mark.parametrize("bad", ("64", 64.0, True, None, -1, 1 << 32))
def test_binding_rejects_tile_cols_before_it_calls_the_library(bad):
    b = Affine4Batch.__new__(Affine4Batch)  # no device needed: the check comes first
    b._h, b.npairs = None, 0
    with pytest.raises(ValueError, match="tile_cols"):
        b.align_tiled(bad)


def test_tiled_needs_trace():
    with pytest.raises(ValueError, match="trace"):
        pa.align_affine4([(b"ACGT", b"ACGT")], DOUBLE, trace=False, tiled=True)


def test_binding_has_the_keys_and_times_of_the_two_layer_route():
    import inspect

    assert list(inspect.signature(Affine4Batch.align_tiled).parameters) == ["self", "tile_cols"]
    assert inspect.signature(Affine4Batch.align_tiled).parameters["tile_cols"].default == 0
    assert list(inspect.signature(pa.align_affine4).parameters) == ["pairs", "cm", "trace", "tiled"]
    src = inspect.getsource(Affine4Batch.tiled_info)
    for key in ("chunks", "rounds", "tile_jobs", "refill_cells", "chunk_bytes_max"):
        assert f'"{key}"' in src and f'"{key}"' in inspect.getsource(pa.AffineBatch.tiled_info)


def test_no_gpu_fails_loudly():
    if capi.load().pa_device_count() > 0:
        return
    with pytest.raises(pa.PaError):
        pa.align_affine4([(b"ACGT", b"AGGT")], DOUBLE, tiled=True)
    with pytest.raises(pa.PaError):
        Affine4Batch([(b"ACGT", b"ACGT")], DOUBLE, trace=True)
