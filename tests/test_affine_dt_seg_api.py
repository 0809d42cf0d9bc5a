"""CPU-side checks of the segmented traceback of the diagonal-transition route: the header's declarations, the exported symbols, the
Python methods' signatures, and the argument checks that run before any device is touched."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from astar_pairwise_aligner_amd import AffineBatch, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
FNS = ("pa_affine_batch_align_dt_seg", "pa_affine_batch_dt_seg_info")


def test_header_declares_the_dt_seg_api():
    txt = re.sub(r"\s+", " ", (ROOT / "include" / "pa_affine_hip.h").read_text())
    for fn in FNS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn), fn
    assert ("int pa_affine_batch_align_dt_seg(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, "
            "int32_t* cost_out, int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* refill_ms, "
            "float* walk_ms);") in txt
    assert ("void pa_affine_batch_dt_seg_info(const pa_affine_batch* ab, double* chunks, double* rounds, double* seg_jobs, "
            "double* refill_cells, double* bytes_max);") in txt
    # the byte formula a test can compute (tests/test_gpu_affine_dt_seg.py does)
    for part in ("(E + 2) L W 4", "(nseg - 1) E L W 4", "(E + S + 1) L W 4", "rounded up to 16", "max(E, ceil(sqrt((s' + 1) E)))"):
        assert part in txt, part


def test_null_batch_is_an_argument_error():
    assert capi.load().pa_affine_batch_align_dt_seg(None, 0, 0, 5, 0, None, None, None, None, None, None, None) == PA_E_ARG
    assert capi.last_error().startswith("pa_affine_batch_align_dt_seg:")
    vals = [capi.C.c_double(7) for _ in range(5)]
    capi.load().pa_affine_batch_dt_seg_info(None, *[capi.C.byref(v) for v in vals])  # no batch: zeros
    assert [v.value for v in vals] == [0] * 5


def test_python_signatures():
    sig = inspect.signature(AffineBatch.align_dt_seg)
    assert list(sig.parameters) == ["self", "s_max", "seg", "free_start", "free_end"]
    assert sig.parameters["seg"].default == 0 and sig.parameters["seg"].default is not False
    assert sig.parameters["free_start"].default is False and sig.parameters["free_end"].default is False
    assert list(inspect.signature(AffineBatch.dt_seg_info).parameters) == ["self"]


def _no_device():
    b = AffineBatch.__new__(AffineBatch)  # no device: the checks come first
    b._h, b.npairs = None, 1
    return b


@pytest.mark.parametrize("bad", (-1, 1 << 30, 1.5, "9", None, True))
def test_bad_s_max_raises_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    with pytest.raises(ValueError, match="s_max"):
        b.align_dt_seg(bad)
    with pytest.raises(ValueError, match="s_max"):
        b.align_dt_seg(bad, 8, True, True)


@pytest.mark.parametrize("bad", (2, -1, 1.0, "1", None))
def test_bad_switches_raise_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    with pytest.raises(ValueError, match="free_start"):
        b.align_dt_seg(5, free_start=bad)
    with pytest.raises(ValueError, match="free_end"):
        b.align_dt_seg(5, 0, False, bad)


@pytest.mark.parametrize("bad", (-1, 1 << 30, 8.0, "8", None, True, False, np.bool_(True)))
def test_bad_seg_raises_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="seg"):
        _no_device().align_dt_seg(5, bad)
    with pytest.raises(ValueError, match="seg"):
        _no_device().align_dt_seg(5, seg=bad, free_start=True)
