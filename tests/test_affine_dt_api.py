"""CPU-side checks of the diagonal-transition route of the gap-affine batch: the header's declarations, the exported symbols, the Python
methods' signatures, and the argument checks and plumbing that run before any device is touched."""
import inspect
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
CM = AffineCost.affine(4, 6, 2)
FNS = ("pa_affine_batch_run_dt", "pa_affine_batch_align_dt", "pa_affine_batch_dt_info")


def test_header_declares_the_dt_api():
    txt = re.sub(r"\s+", " ", (ROOT / "include" / "pa_affine_hip.h").read_text())
    for fn in FNS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn), fn
    assert "int pa_affine_batch_run_dt(pa_affine_batch* ab, int32_t s_max, int32_t* cost_out, float* kernel_ms);" in txt
    assert ("int pa_affine_batch_align_dt(pa_affine_batch* ab, int32_t s_max, int32_t* cost_out, char** cigar_out, float* forward_ms, "
            "float* trace_ms);") in txt
    assert ("void pa_affine_batch_dt_info(const pa_affine_batch* ab, double* found, double* not_found, double* chunks, double* front_cells, "
            "double* extend_chars, double* bytes_max);") in txt


def test_the_unit_is_built():
    from astar_pairwise_aligner_amd import _build

    assert "affine_dt_unit.hip" in _build.HIP_SOURCES
    assert (ROOT / "astar-pairwise-aligner_amd" / "csrc" / "affine_dt_kernel.hpp").exists()


@pytest.mark.parametrize("fn", FNS[:2])
def test_null_batch_is_an_argument_error(fn):
    args = (None, 5, None, None) if fn.endswith("run_dt") else (None, 5, None, None, None, None)
    assert getattr(capi.load(), fn)(*args) == PA_E_ARG
    assert capi.last_error().startswith(fn + ":")


def test_dt_info_of_a_null_batch_is_zero():
    import ctypes as C

    vals = [C.c_double(7) for _ in range(6)]
    capi.load().pa_affine_batch_dt_info(None, *[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0.0] * 6


def test_python_signatures():
    assert list(inspect.signature(AffineBatch.run_dt).parameters) == ["self", "s_max"]
    assert list(inspect.signature(AffineBatch.align_dt).parameters) == ["self", "s_max"]
    assert list(inspect.signature(AffineBatch.dt_info).parameters) == ["self"]
    sig = inspect.signature(pa.align_affine)
    assert list(sig.parameters) == ["pairs", "cm", "tiled", "chain", "s_max"] and sig.parameters["s_max"].default is None


class _Stub:
    """Stands in for AffineBatch: records what align_affine asks of it."""
    calls = []

    def __init__(self, pairs, cm, trace=False, chain=False, **kw):
        _Stub.calls.append(("init", len(pairs), trace, chain, kw))

    def align(self):
        _Stub.calls.append(("align",))
        return ["old"]

    def align_tiled(self):
        _Stub.calls.append(("align_tiled",))
        return ["tiled"]

    def align_dt(self, s_max):
        _Stub.calls.append(("align_dt", s_max))
        return ["dt"]

    def close(self):
        _Stub.calls.append(("close",))


def test_align_affine_plumbing(monkeypatch):
    monkeypatch.setattr(capi, "AffineBatch", _Stub)
    pairs = [(b"ACGT", b"ACG")]
    _Stub.calls.clear()
    assert pa.align_affine(pairs, CM) == ["old"]  # without s_max: the old path
    assert _Stub.calls == [("init", 1, True, False, {}), ("align",), ("close",)]
    _Stub.calls.clear()
    assert pa.align_affine(pairs, CM, tiled=True) == ["tiled"]
    assert _Stub.calls == [("init", 1, True, False, {}), ("align_tiled",), ("close",)]
    _Stub.calls.clear()
    assert pa.align_affine(pairs, CM, s_max=17) == ["dt"]
    assert _Stub.calls == [("init", 1, True, False, {}), ("align_dt", 17), ("close",)]
    _Stub.calls.clear()
    assert pa.align_affine(pairs, CM, s_max=0) == ["dt"]  # 0 is a bound, not "no bound"
    assert _Stub.calls[1] == ("align_dt", 0)
    for kw in ({"tiled": True}, {"chain": True}, {"tiled": True, "chain": True}):
        with pytest.raises(ValueError, match="s_max"):
            pa.align_affine(pairs, CM, s_max=5, **kw)


@pytest.mark.parametrize("bad", (-1, 1 << 30, 1.5, "9", None, True))
def test_bad_s_max_raises_before_the_library_is_called(bad):
    b = AffineBatch.__new__(AffineBatch)  # no device: _s_max comes first
    b._h, b.npairs = None, 1
    for call in (b.run_dt, b.align_dt):
        with pytest.raises(ValueError, match="s_max"):
            call(bad)
