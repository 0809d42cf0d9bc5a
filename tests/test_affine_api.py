"""CPU-side checks of the gap-affine batch API: the binding's argument checks, the C ABI's own checks (they run before any device is
touched), the loud failure without a GPU, and the header's declarations."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent


def test_constructors_mirror_the_reference():
    assert (AffineCost.lcs().sub, AffineCost.lcs().ins, AffineCost.lcs().del_, AffineCost.lcs().layers) == (None, 1, 1, [])
    assert (AffineCost.unit().sub, AffineCost.unit().ins, AffineCost.unit().del_) == (1, 1, 1)
    assert AffineCost.affine(4, 6, 2).layers == [("ins", 6, 2), ("del", 6, 2)]
    cm = AffineCost.affine_asymmetric(5, 3, 1, 7, 2)
    assert (cm.sub, cm.ins, cm.del_, cm.layers) == (5, None, None, [("ins", 3, 1), ("del", 7, 2)])
    c = AffineCost.linear_affine(3, 2, 4, 1).to_c()
    assert (c.sub, c.ins, c.del_, c.ins_open, c.ins_extend, c.del_open, c.del_extend) == (3, 2, 2, 4, 1, 4, 1)
    assert AffineCost.affine(4, 6, 2).max_edge() == 8


@pytest.mark.parametrize("cm", [AffineCost(0, 1, 1), AffineCost.linear(1, 1001), AffineCost.affine(4, 0, 2),
                                AffineCost(1, None, 1), AffineCost(1, 1, None), AffineCost.double_affine(4, 6, 2, 20, 1),
                                AffineCost(1, None, None, [("del", 1, 1), ("ins", 1, 1)]), AffineCost.linear(1.5, 1)])
def test_binding_rejects_cost_models(cm):
    with pytest.raises(ValueError):
        AffineBatch([(b"A", b"A")], cm)


def test_binding_rejects_bad_pairs():
    with pytest.raises(ValueError):
        AffineBatch([("ACGT", b"ACGT")], AffineCost.unit())
    with pytest.raises(ValueError):
        AffineBatch([(b"A", b"A")], "unit")
    with pytest.raises(ValueError):  # (|a| + |b| + 1) * 1000 >= 2^30
        AffineBatch([(b"A" * 600000, b"A" * 600000)], AffineCost.linear(1000, 1000))


def _create(cost, a=b"ACGT", b=b"ACGT"):
    L = capi.load()
    ap = (C.c_char_p * 1)(a)
    bp = (C.c_char_p * 1)(b)
    al, bl = np.array([len(a)], np.uint64), np.array([len(b)], np.uint64)
    c = capi._AffineCostC(*cost)
    return L.pa_affine_batch_create(ap, capi._p(al), bp, capi._p(bl), 1, C.byref(c), 0)


@pytest.mark.parametrize("cost", [(0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0), (1, 0, 1, 0, 0, 0, 0), (1, 1, 1, 0, 0, 1001, 1),
                                  (-1, 1, 1, 0, 0, 0, 0), (1, 0, 0, 6, 0, 6, 2), (1, 0, 0, 6, 2, 0, 2)])
def test_c_abi_rejects_cost_models(cost):
    assert not _create(cost)
    assert capi.last_error().startswith("pa_affine_batch_create:")


def test_c_abi_rejects_overflow_sized_pairs():
    big = b"A" * 600000
    assert not _create((1000, 1000, 1000, 0, 0, 0, 0), big, big)
    msg = capi.last_error()
    assert "pair 0" in msg and "2^30" in msg


def test_no_gpu_fails_loudly():
    if capi.load().pa_device_count() > 0:
        return
    with pytest.raises(pa.PaError):
        AffineBatch([(b"ACGT", b"ACGT")], AffineCost.affine(4, 6, 2))
    with pytest.raises(pa.PaError):
        pa.align_affine([(b"ACGT", b"AGGT")], AffineCost.unit())


def test_header_declares_the_api():
    txt = (ROOT / "include" / "pa_affine_hip.h").read_text()
    body = re.search(r"typedef struct pa_affine_cost\s*\{(.*?)\}\s*pa_affine_cost;", txt, flags=re.S).group(1)
    assert [f.strip() for f in body.replace("int32_t", "").replace(";", "").split(",")] == [
        "sub", "ins", "del", "ins_open", "ins_extend", "del_open", "del_extend"]
    for fn in ("pa_affine_batch_create", "pa_affine_batch_run", "pa_affine_batch_align", "pa_affine_batch_info", "pa_affine_batch_destroy"):
        assert re.search(r"\b" + fn + r"\(", txt), fn
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn)
    assert [f for f, _ in capi._AffineCostC._fields_] == ["sub", "ins", "del_", "ins_open", "ins_extend", "del_open", "del_extend"]
