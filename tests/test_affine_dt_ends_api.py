"""CPU-side checks of the ends-free diagonal-transition route of the gap-affine batch: the header's declarations, the exported symbols,
the Python methods' signatures, and the argument checks and plumbing that run before any device is touched."""
import inspect
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
CM = AffineCost.affine(4, 6, 2)
FNS = ("pa_affine_batch_run_dt_ends", "pa_affine_batch_align_dt_ends")


def test_header_declares_the_dt_ends_api():
    txt = re.sub(r"\s+", " ", (ROOT / "include" / "pa_affine_hip.h").read_text())
    for fn in FNS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn), fn
    assert ("int pa_affine_batch_run_dt_ends(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, "
            "int64_t* end_out, float* kernel_ms);") in txt
    assert ("int pa_affine_batch_align_dt_ends(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, "
            "int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* trace_ms);") in txt


@pytest.mark.parametrize("fn", FNS)
def test_null_batch_is_an_argument_error(fn):
    args = (None, 1, 1, 5, None, None, None) if fn.endswith("run_dt_ends") else (None, 1, 1, 5, None, None, None, None, None, None)
    assert getattr(capi.load(), fn)(*args) == PA_E_ARG
    assert capi.last_error().startswith(fn + ":")


def test_python_signatures():
    for fn in (AffineBatch.run_dt_ends, AffineBatch.align_dt_ends):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["self", "s_max", "free_start", "free_end"]
        assert sig.parameters["free_start"].default is True and sig.parameters["free_end"].default is True
    sig = inspect.signature(pa.map_affine)
    assert list(sig.parameters) == ["pairs", "cm", "free_start", "free_end", "tiled", "chain", "s_max"] and sig.parameters["s_max"].default is None
    assert pa.map_affine is capi.map_affine


def _no_device():
    b = AffineBatch.__new__(AffineBatch)  # no device: the checks come first
    b._h, b.npairs = None, 1
    return b


@pytest.mark.parametrize("bad", (-1, 1 << 30, 1.5, "9", None, True))
def test_bad_s_max_raises_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    for call in (b.run_dt_ends, b.align_dt_ends):
        with pytest.raises(ValueError, match="s_max"):
            call(bad)
        with pytest.raises(ValueError, match="s_max"):
            call(bad, False, True)
    if bad is not None:  # (None is map_affine's "no bound": the DP route)
        with pytest.raises(ValueError, match="s_max"):
            pa.map_affine([(b"ACGT", b"ACG")], CM, s_max=bad)


@pytest.mark.parametrize("bad", (2, -1, 1.0, "1", None))
def test_bad_switches_raise_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    for call in (b.run_dt_ends, b.align_dt_ends):
        with pytest.raises(ValueError, match="free_start"):
            call(5, free_start=bad)
        with pytest.raises(ValueError, match="free_end"):
            call(5, free_end=bad)
    with pytest.raises(ValueError, match="free_end"):
        pa.map_affine([(b"ACGT", b"ACG")], CM, free_end=bad, s_max=5)


class _Stub:
    """Stands in for AffineBatch: records what map_affine asks of it."""
    calls = []

    def __init__(self, pairs, cm, trace=False, chain=False, **kw):
        _Stub.calls.append(("init", len(pairs), trace, chain, kw))

    def align(self):
        _Stub.calls.append(("align",))
        return [(3, "old")]

    def align_tiled(self):
        _Stub.calls.append(("align_tiled",))
        return [(3, "tiled")]

    def ends(self):
        import numpy as np

        _Stub.calls.append(("ends",))
        return np.array([[1, 4]])

    def align_dt_ends(self, s_max, free_start=True, free_end=True):
        _Stub.calls.append(("align_dt_ends", s_max, free_start, free_end))
        return ["dt"]

    def close(self):
        _Stub.calls.append(("close",))


def test_map_affine_plumbing(monkeypatch):
    monkeypatch.setattr(capi, "AffineBatch", _Stub)
    pairs = [(b"ACGT", b"ACG")]
    _Stub.calls.clear()
    assert pa.map_affine(pairs, CM) == [(3, "old", 1, 4)]  # without s_max: the old path, the switches set on the batch
    assert _Stub.calls == [("init", 1, True, False, {"free_start": 1, "free_end": 1}), ("align",), ("ends",), ("close",)]
    _Stub.calls.clear()
    assert pa.map_affine(pairs, CM, s_max=17) == ["dt"]  # with it: the switches go with the call, the batch stays global
    assert _Stub.calls == [("init", 1, True, False, {}), ("align_dt_ends", 17, 1, 1), ("close",)]
    _Stub.calls.clear()
    assert pa.map_affine(pairs, CM, free_start=False, s_max=0) == ["dt"]  # 0 is a bound, not "no bound"
    assert _Stub.calls[1] == ("align_dt_ends", 0, 0, 1)
    for kw in ({"tiled": True}, {"chain": True}, {"tiled": True, "chain": True}):
        with pytest.raises(ValueError, match="s_max"):
            pa.map_affine(pairs, CM, s_max=5, **kw)
