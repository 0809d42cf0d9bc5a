"""CPU-side checks of the chained route of the double-affine batch: the new header's declarations, the exported symbols, the C ABI's own
argument checks (they run before any device is touched), and the Python signatures."""
import ctypes as C
import inspect
import re
from pathlib import Path

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, _build, capi

ROOT = Path(__file__).resolve().parent.parent
FUNCS = ("pa_affine4_batch_set_chain", "pa_affine4_batch_chain_info")


def squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_exactly_the_two_functions():
    txt = (ROOT / "include" / "pa_affine4_chain_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert '#include "pa_affine4_hip.h"' in code
    assert set(re.findall(r"\b(pa_[a-z_0-9]+)\s*\(", code)) == set(FUNCS)
    flat = squash(code)
    assert flat.count(";") == 2  # two declarations and nothing else
    assert "int pa_affine4_batch_set_chain(pa_affine4_batch* ab, int on);" in flat
    assert ("void pa_affine4_batch_chain_info(const pa_affine4_batch* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks, "
            "double* bnd_bytes_max);") in flat
    comment = squash(txt)
    assert "(strips - 1) * (|a| + 1) * 16 bytes" in comment  # the memory formula
    assert "bounded time" in comment and "PA_E_INTERNAL" in comment  # the bounded wait
    # the existing headers keep their function lists and point here
    for name in ("pa_affine4_hip.h", "pa_affine4_tiled_hip.h"):
        other = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)
        assert not set(re.findall(r"\b(pa_[a-z_0-9]+)\s*\(", other)) & set(FUNCS)
    assert "pa_affine4_chain_hip.h" in (ROOT / "include" / "pa_affine4_hip.h").read_text()


def test_symbols_are_exported_and_built():
    L = capi.load()
    for fn in FUNCS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(L, fn)
    assert (_build.CSRC / "affine4_chain_kernel.hpp").exists() and (_build.CSRC / "affine4_chain_value.hpp").exists()


def test_c_abi_checks_a_null_batch():
    L = capi.load()
    assert L.pa_affine4_batch_set_chain(None, 1) == -4  # PA_E_ARG
    assert capi.last_error().startswith("pa_affine4_batch_set_chain:")
    assert L.pa_affine4_batch_set_chain(None, 2) == -4
    L.pa_affine4_batch_chain_info(None, None, None, None, None, None)  # NULLs everywhere
    vals = [C.c_double(7) for _ in range(5)]
    L.pa_affine4_batch_chain_info(None, *[C.byref(v) for v in vals])
    assert [v.value for v in vals] == [0, 0, 0, 0, 0]
    some = [C.c_double(7) for _ in range(2)]
    L.pa_affine4_batch_chain_info(None, None, C.byref(some[0]), None, None, C.byref(some[1]))
    assert [v.value for v in some] == [0, 0]


def test_python_signatures():
    p = inspect.signature(Affine4Batch.__init__).parameters
    assert list(p) == ["self", "pairs", "cm", "trace", "chain"] and p["chain"].default is False and p["trace"].default is False
    assert list(inspect.signature(pa.align_affine4).parameters) == ["pairs", "cm", "trace", "tiled"]
    assert list(inspect.signature(Affine4Batch.align_tiled).parameters) == ["self", "tile_cols"]
    for name in ("set_chain", "chain_info"):
        assert callable(getattr(Affine4Batch, name)) and callable(getattr(pa.AffineBatch, name))
    assert list(inspect.signature(Affine4Batch.set_chain).parameters) == ["self", "on"]
