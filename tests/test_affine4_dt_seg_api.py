"""CPU-side checks of the segmented traceback of the double-affine diagonal-transition route: the new header's declarations, the
exported and bound symbols, the Python methods' signatures, and the argument checks that run before any device is touched."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
FNS = ("pa_affine4_batch_align_dt_seg", "pa_affine4_batch_dt_seg_info")


def _code(name):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S))


def test_header_declares_exactly_the_dt_seg_api():
    code = _code("pa_affine4_dt_seg_hip.h")
    assert sorted(re.findall(r"\b(pa_\w+)\(", code)) == sorted(FNS)
    assert '#include "pa_affine4_hip.h"' in code
    assert ("int pa_affine4_batch_align_dt_seg(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, "
            "int32_t* cost_out, int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* refill_ms, "
            "float* walk_ms);") in code
    assert ("void pa_affine4_batch_dt_seg_info(const pa_affine4_batch* ab, double* chunks, double* rounds, double* seg_jobs, "
            "double* refill_cells, double* bytes_max);") in code
    # the two-layer functions, with the other batch type
    two = _code("pa_affine_hip.h")
    for fn in FNS:
        decl = re.search(r"\b(?:int|void) " + fn + r"\([^)]*\);", code).group(0)
        assert decl.replace("pa_affine4_batch", "pa_affine_batch") in two, fn
    # the byte formula a test can compute (tests/test_gpu_affine4_dt_seg.py does), and the argument's terms
    txt = re.sub(r"\s+", " ", (ROOT / "include" / "pa_affine4_dt_seg_hip.h").read_text())
    for part in ("(E + 1) + sum of (e_t + 1) + 1 rows", "(nseg - 1) H rows", "H + 5 S + 1 rows", "rounded up to 16", "and 40",
                 "5 S^2 >= (s' + 1) H", "H = E + e_0 + e_1 + e_2 + e_3", "Ew = max(E, e_0, .., e_3)", "max(Ew, s' + 1)"):
        assert part in txt, part


def test_the_other_headers_declare_none_of_it():
    for name in ("pa_affine4_hip.h", "pa_affine4_dt_hip.h", "pa_affine4_tiled_hip.h", "pa_affine4_chain_hip.h", "pa_affine4_ends_hip.h", "pa_affine_hip.h"):
        code = _code(name)
        assert not any(re.search(r"\b" + fn + r"\(", code) for fn in FNS), name
    main = (ROOT / "include" / "pa_affine4_hip.h").read_text()
    assert "pa_affine4_dt_seg_hip.h" in main and re.search(r"Not supported:[^.]*diagonal-transition", main)
    assert "without a segmented" not in re.sub(r"\s+", " ", main)


def test_symbols_are_exported_and_bound():
    L = capi.load()
    for fn in FNS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(L, fn), fn
    assert "affine4_dt_seg_unit.hip" in pa._build.HIP_SOURCES
    assert len(L.pa_affine4_batch_align_dt_seg.argtypes) == 12 and L.pa_affine4_batch_align_dt_seg.argtypes[4] is capi.C.c_uint32
    assert len(L.pa_affine4_batch_dt_seg_info.argtypes) == 6 and L.pa_affine4_batch_dt_seg_info.restype is None


def test_null_batch_is_an_argument_error():
    assert capi.load().pa_affine4_batch_align_dt_seg(None, 0, 0, 5, 0, None, None, None, None, None, None, None) == PA_E_ARG
    assert capi.last_error().startswith("pa_affine4_batch_align_dt_seg:")
    vals = [capi.C.c_double(7) for _ in range(5)]
    capi.load().pa_affine4_batch_dt_seg_info(None, *[capi.C.byref(v) for v in vals])  # no batch: zeros
    assert [v.value for v in vals] == [0] * 5


def test_python_signatures():
    sig = inspect.signature(Affine4Batch.align_dt_segmented)
    assert list(sig.parameters) == ["self", "s_max", "seg", "free_start", "free_end"]
    assert sig.parameters["seg"].default == 0 and sig.parameters["seg"].default is not False
    assert sig.parameters["free_start"].default is False and sig.parameters["free_end"].default is False
    assert list(inspect.signature(Affine4Batch.dt_segmented_info).parameters) == ["self"]
    # the arguments and defaults of AffineBatch.align_dt_seg, under the name the double-affine batch is free to take
    assert str(sig) == str(inspect.signature(AffineBatch.align_dt_seg))
    assert not hasattr(Affine4Batch, "align_dt_seg") and not hasattr(Affine4Batch, "dt_seg_info")
    assert not hasattr(AffineBatch, "align_dt_segmented")
    # what the existing tests pin stays
    assert list(inspect.signature(Affine4Batch.__init__).parameters) == ["self", "pairs", "cm", "trace", "chain"]
    assert list(inspect.signature(pa.map_affine_dt).parameters) == ["pairs", "cm", "s_max", "free_start", "free_end"]
    doc = re.sub(r"\s+", " ", Affine4Batch.__doc__)
    assert "align_dt_segmented" in doc and "Not supported" not in doc


def _no_device():
    b = Affine4Batch.__new__(Affine4Batch)  # no device: the checks come first
    b._h, b.npairs = None, 1
    return b


@pytest.mark.parametrize("bad", (-1, 1 << 30, 1.5, "9", None, True))
def test_bad_s_max_raises_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    with pytest.raises(ValueError, match="s_max"):
        b.align_dt_segmented(bad)
    with pytest.raises(ValueError, match="s_max"):
        b.align_dt_segmented(bad, 30, True, True)


@pytest.mark.parametrize("bad", (2, -1, 1.0, "1", None))
def test_bad_switches_raise_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    with pytest.raises(ValueError, match="free_start"):
        b.align_dt_segmented(5, free_start=bad)
    with pytest.raises(ValueError, match="free_end"):
        b.align_dt_segmented(5, 0, False, bad)


@pytest.mark.parametrize("bad", (-1, 1 << 30, 8.0, "8", None, True, False, np.bool_(True)))
def test_bad_seg_raises_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="seg"):
        _no_device().align_dt_segmented(5, bad)
    with pytest.raises(ValueError, match="seg"):
        _no_device().align_dt_segmented(5, seg=bad, free_start=True)
