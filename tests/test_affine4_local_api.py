"""CPU-side checks of local alignment over the double-affine batch: the header's declarations, the exported symbols, the Python methods'
signatures, and the argument checks that run before any device is touched."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
FNS = ("pa_affine4_batch_run_local", "pa_affine4_batch_align_local", "pa_affine4_batch_local_info")
DOUBLE = AffineCost.double_affine(4, 6, 2, 24, 1)


def test_header_declares_the_local_api():
    txt = (ROOT / "include" / "pa_affine4_local_hip.h").read_text()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert sorted(re.findall(r"\b(pa_\w+)\(", code)) == sorted(FNS)
    assert '#include "pa_affine4_hip.h"' in code
    assert ("int pa_affine4_batch_run_local(pa_affine4_batch* ab, int32_t match, int32_t* score_out, int64_t* a_end_out, int64_t* b_end_out, "
            "float* kernel_ms);") in code
    assert ("int pa_affine4_batch_align_local(pa_affine4_batch* ab, int32_t match, int32_t* score_out, int64_t* a_start_out, int64_t* a_end_out, "
            "int64_t* b_start_out, int64_t* b_end_out, char** cigar_out, float* forward_ms, float* trace_ms);") in code
    assert "void pa_affine4_batch_local_info(const pa_affine4_batch* ab, double* chunks, double* bytes_max);" in code
    # the declarations live in the header of their own, which says what is out of scope; the two-layer header points here
    assert "_local" not in (ROOT / "include" / "pa_affine4_hip.h").read_text()
    for word in ("tiled", "chained", "diagonal transition", "banded"):
        assert word in txt, word
    assert "pa_affine4_local_hip.h" in (ROOT / "include" / "pa_affine_local_hip.h").read_text()


def test_symbols_are_exported_and_bound():
    L = capi.load()
    for fn in FNS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(L, fn), fn
    assert "affine4_local_unit.hip" in pa._build.HIP_SOURCES
    assert (pa._build.CSRC / "affine4_local_unit.hip").exists() and (pa._build.CSRC / "affine4_local_kernel.hpp").exists()
    assert len(L.pa_affine4_batch_run_local.argtypes) == 6 and L.pa_affine4_batch_run_local.argtypes[1] is C.c_int32
    assert len(L.pa_affine4_batch_align_local.argtypes) == 10 and L.pa_affine4_batch_align_local.argtypes[1] is C.c_int32
    assert len(L.pa_affine4_batch_local_info.argtypes) == 3 and L.pa_affine4_batch_local_info.restype is None


@pytest.mark.parametrize("fn", FNS[:2])
def test_null_batch_is_an_argument_error(fn):
    args = (None, 2) + (None,) * (4 if fn.endswith("run_local") else 8)
    assert getattr(capi.load(), fn)(*args) == PA_E_ARG
    assert capi.last_error().startswith(fn + ":")


def test_local_info_of_a_null_batch_is_zero():
    vals = [C.c_double(7) for _ in range(2)]
    capi.load().pa_affine4_batch_local_info(None, *[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0.0, 0.0]


def test_python_signatures():
    assert list(inspect.signature(Affine4Batch.run_sw).parameters) == ["self", "match"]
    assert list(inspect.signature(Affine4Batch.align_sw).parameters) == ["self", "match"]
    assert list(inspect.signature(Affine4Batch.sw_info).parameters) == ["self"]
    assert list(inspect.signature(pa.align_local).parameters) == ["pairs", "cm", "match"]
    for name in ("run_sw", "align_sw", "sw_info"):  # on Affine4Batch only
        assert not hasattr(capi.AffineBatch, name) and not hasattr(capi._AffineBatchBase, name)


@pytest.mark.parametrize("bad", (True, 1.5, "2", None, 0, 1001, -3))
def test_bad_match_raises_before_the_library_is_called(bad, monkeypatch):
    def no_load(*a, **kw):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(capi, "load", no_load)
    b = Affine4Batch.__new__(Affine4Batch)  # no device: the check of match comes first
    b._h, b.npairs = None, 1
    for call in (b.run_sw, b.align_sw):
        with pytest.raises(ValueError, match="match"):
            call(bad)
    with pytest.raises(ValueError, match="match"):
        pa.align_local([(b"ACGT", b"ACG")], DOUBLE, bad)
