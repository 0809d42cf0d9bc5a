"""CPU-side checks of the diagonal-transition route of the double-affine batch: the new header's declarations, the exported symbols, the
Python methods' signatures, and the argument checks of the C ABI, of Affine4Batch and of map_affine_dt that run before any device is
touched."""
import inspect
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
CM = AffineCost.double_affine(4, 6, 2, 24, 1)
FUNCTIONS = ("pa_affine4_batch_run_dt", "pa_affine4_batch_run_dt_ends", "pa_affine4_batch_align_dt", "pa_affine4_batch_align_dt_ends",
             "pa_affine4_batch_dt_info")
METHODS = ("run_dt", "align_dt", "run_dt_ends", "align_dt_ends", "dt_info")
NULL_ARGS = {
    "pa_affine4_batch_run_dt": (None, 5, None, None),
    "pa_affine4_batch_run_dt_ends": (None, 1, 1, 5, None, None, None),
    "pa_affine4_batch_align_dt": (None, 5, None, None, None, None),
    "pa_affine4_batch_align_dt_ends": (None, 1, 1, 5, None, None, None, None, None, None),
}


def _code(name):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S))


def test_header_declares_exactly_the_dt_api():
    code = _code("pa_affine4_dt_hip.h")
    assert sorted(re.findall(r"\b(pa_\w+)\(", code)) == sorted(FUNCTIONS)
    assert '#include "pa_affine4_hip.h"' in code
    assert "int pa_affine4_batch_run_dt(pa_affine4_batch* ab, int32_t s_max, int32_t* cost_out, float* kernel_ms);" in code
    assert ("int pa_affine4_batch_run_dt_ends(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, "
            "int64_t* end_out, float* kernel_ms);") in code
    assert ("int pa_affine4_batch_align_dt(pa_affine4_batch* ab, int32_t s_max, int32_t* cost_out, char** cigar_out, float* forward_ms, "
            "float* trace_ms);") in code
    assert ("int pa_affine4_batch_align_dt_ends(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, "
            "int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* trace_ms);") in code
    assert ("void pa_affine4_batch_dt_info(const pa_affine4_batch* ab, double* found, double* not_found, double* chunks, double* front_cells, "
            "double* extend_chars, double* bytes_max);") in code
    # the two-layer functions, with the other batch type
    two = _code("pa_affine_hip.h")
    for fn in FUNCTIONS:
        decl = re.search(r"\b(?:int|void) " + fn + r"\([^)]*\);", code).group(0)
        assert decl.replace("pa_affine4_batch", "pa_affine_batch") in two, fn


def test_the_other_affine4_headers_declare_none_of_it():
    for name in ("pa_affine4_hip.h", "pa_affine4_tiled_hip.h", "pa_affine4_chain_hip.h", "pa_affine4_ends_hip.h"):
        code = _code(name)
        assert not any(re.search(r"\b" + fn + r"\(", code) for fn in FUNCTIONS), name
    main = (ROOT / "include" / "pa_affine4_hip.h").read_text()
    assert "pa_affine4_dt_hip.h" in main and re.search(r"Not supported:[^.]*diagonal-transition", main)


def test_symbols_are_exported_and_bound():
    L = capi.load()
    for fn in FUNCTIONS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(L, fn), fn
    assert "affine4_dt_unit.hip" in pa._build.HIP_SOURCES
    assert pa.map_affine_dt is capi.map_affine_dt


@pytest.mark.parametrize("fn", sorted(NULL_ARGS))
def test_null_batch_is_an_argument_error(fn):
    assert getattr(capi.load(), fn)(*NULL_ARGS[fn]) == PA_E_ARG
    assert capi.last_error().startswith(fn + ":")


def test_dt_info_of_a_null_batch_is_zero():
    import ctypes as C

    vals = [C.c_double(7) for _ in range(6)]
    capi.load().pa_affine4_batch_dt_info(None, *[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0.0] * 6


def test_python_signatures():
    for name in METHODS:
        assert getattr(Affine4Batch, name) is getattr(AffineBatch, name), name  # one text over self._fn
    assert list(inspect.signature(Affine4Batch.run_dt).parameters) == ["self", "s_max"]
    assert list(inspect.signature(Affine4Batch.align_dt).parameters) == ["self", "s_max"]
    for fn in (Affine4Batch.run_dt_ends, Affine4Batch.align_dt_ends):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["self", "s_max", "free_start", "free_end"]
        assert sig.parameters["free_start"].default is True and sig.parameters["free_end"].default is True
    assert list(inspect.signature(Affine4Batch.dt_info).parameters) == ["self"]
    sig = inspect.signature(pa.map_affine_dt)
    assert list(sig.parameters) == ["pairs", "cm", "s_max", "free_start", "free_end"]
    assert sig.parameters["s_max"].default is inspect.Parameter.empty
    assert sig.parameters["free_start"].default is True and sig.parameters["free_end"].default is True
    # what the existing tests pin stays
    assert list(inspect.signature(Affine4Batch.__init__).parameters) == ["self", "pairs", "cm", "trace", "chain"]
    assert list(inspect.signature(pa.align_affine4).parameters) == ["pairs", "cm", "trace", "tiled"]
    assert not hasattr(Affine4Batch, "align_dt_seg")


def _no_device():
    b = Affine4Batch.__new__(Affine4Batch)  # no device: the checks come first
    b._h, b.npairs = None, 1
    return b


@pytest.mark.parametrize("bad", (-1, 1 << 30, 1.5, "9", None, True))
def test_bad_s_max_raises_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    for call in (b.run_dt, b.align_dt, b.run_dt_ends, b.align_dt_ends):
        with pytest.raises(ValueError, match="s_max"):
            call(bad)
    with pytest.raises(ValueError, match="s_max"):
        pa.map_affine_dt([(b"ACGT", b"ACG")], CM, bad)
    with pytest.raises(ValueError, match="s_max"):
        pa.map_affine_dt([(b"ACGT", b"ACG")], AffineCost.affine(4, 6, 2), bad)


@pytest.mark.parametrize("bad", (2, -1, 1.0, "1", None))
def test_bad_switches_raise_before_the_library_is_called(bad, monkeypatch):
    monkeypatch.setattr(capi, "load", lambda *a, **k: pytest.fail("the library was called"))
    b = _no_device()
    for call in (b.run_dt_ends, b.align_dt_ends):
        with pytest.raises(ValueError, match="free_start"):
            call(5, free_start=bad)
        with pytest.raises(ValueError, match="free_end"):
            call(5, free_end=bad)
    with pytest.raises(ValueError, match="free_start"):
        pa.map_affine_dt([(b"ACGT", b"ACG")], CM, 5, free_start=bad)
    with pytest.raises(ValueError, match="free_end"):
        pa.map_affine_dt([(b"ACGT", b"ACG")], CM, 5, free_end=bad)


class _Stub:
    """Stands in for either batch: records what map_affine_dt asks of it."""
    calls = []

    def __init__(self, pairs, cm, trace=False, **kw):
        _Stub.calls.append((type(self).__name__, len(pairs), trace, kw))

    def align_dt_ends(self, s_max, free_start=True, free_end=True):
        _Stub.calls.append(("align_dt_ends", s_max, free_start, free_end))
        return ["dt"]

    def close(self):
        _Stub.calls.append(("close",))


class _Stub4(_Stub):
    pass


def test_map_affine_dt_picks_the_batch_by_the_layers(monkeypatch):
    monkeypatch.setattr(capi, "AffineBatch", _Stub)
    monkeypatch.setattr(capi, "Affine4Batch", _Stub4)
    pairs = [(b"ACGT", b"ACG")]
    _Stub.calls.clear()
    assert pa.map_affine_dt(pairs, CM, 17) == ["dt"]
    assert _Stub.calls == [("_Stub4", 1, True, {}), ("align_dt_ends", 17, 1, 1), ("close",)]
    _Stub.calls.clear()
    assert pa.map_affine_dt(pairs, AffineCost.affine(4, 6, 2), 0, free_start=False) == ["dt"]
    assert _Stub.calls == [("_Stub", 1, True, {}), ("align_dt_ends", 0, 0, 1), ("close",)]
    _Stub.calls.clear()
    assert pa.map_affine_dt(pairs, AffineCost.unit(), 3, False, False) == ["dt"]
    assert _Stub.calls[0][0] == "_Stub" and _Stub.calls[1] == ("align_dt_ends", 3, 0, 0)
    with pytest.raises(ValueError, match="AffineCost"):
        pa.map_affine_dt(pairs, None, 3)
    # map_affine keeps its refusal (tests/test_affine4_ends_api.py pins the message)
    with pytest.raises(ValueError, match="diagonal transition has no double-affine route"):
        pa.map_affine(pairs, CM, s_max=10)
