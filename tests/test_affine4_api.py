"""CPU-side checks of the double-affine batch API: the binding's argument checks, the C ABI's own checks (they run before any device is
touched), the loud failure without a GPU, the header's declarations, and AffineBatch's unchanged refusal of four layers."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
FUNCS = ("pa_affine4_batch_create", "pa_affine4_batch_run", "pa_affine4_batch_align", "pa_affine4_batch_info", "pa_affine4_batch_destroy")


def four(sub=4, ins=None, del_=None, layers=((6, 2), (6, 2), (24, 1), (24, 1))):
    return AffineCost(sub, ins, del_, [(k, o, e) for k, (o, e) in zip(["ins", "del", "ins", "del"], layers)])


def test_to_c4_mirrors_the_model():
    c = AffineCost.double_affine(4, 6, 2, 24, 1).to_c4()
    assert (c.sub, c.ins, c.del_, list(c.open), list(c.extend)) == (4, 0, 0, [6, 6, 24, 24], [2, 2, 1, 1])
    c = four(None, 5, 3, ((1, 2), (3, 4), (5, 6), (7, 8))).to_c4()
    assert (c.sub, c.ins, c.del_, list(c.open), list(c.extend)) == (0, 5, 3, [1, 3, 5, 7], [2, 4, 6, 8])
    assert AffineCost.double_affine(4, 6, 2, 24, 1).max_edge() == 25
    assert "Affine4Batch" in AffineCost.double_affine.__doc__


@pytest.mark.parametrize("cm", [
    AffineCost.affine(4, 6, 2), AffineCost.unit(), AffineCost.lcs(),  # not four layers
    AffineCost(1, None, None, [("del", 1, 1), ("ins", 1, 1), ("ins", 2, 1), ("del", 2, 1)]),  # another order
    AffineCost(1, None, None, [("ins", 1, 1), ("del", 1, 1), ("ins", 2, 1)]),
    AffineCost(1, None, None, [("ins", 1, 1), ("del", 1, 1), ("ins", 2, 1), ("del", 2, 1), ("ins", 3, 1)]),
    four(0), four(1001), four(1.5), four(4, 0), four(4, None, 1001),
    four(layers=((0, 2), (6, 2), (24, 1), (24, 1))), four(layers=((6, 2), (6, 2), (24, 1), (24, 1001))),
    four(layers=((6, 2), (6, None), (24, 1), (24, 1))), four(layers=((6, 2), (6, 2), (24.0, 1), (24, 1))),
])
def test_binding_rejects_cost_models(cm):
    with pytest.raises(ValueError):
        cm.to_c4()
    with pytest.raises(ValueError):
        Affine4Batch([(b"A", b"A")], cm)


def test_binding_rejects_bad_pairs():
    cm = AffineCost.double_affine(4, 6, 2, 24, 1)
    with pytest.raises(ValueError):
        Affine4Batch([("ACGT", b"ACGT")], cm)
    with pytest.raises(ValueError):
        Affine4Batch([(b"A", b"A")], "double_affine")
    with pytest.raises(ValueError, match="pair 1"):  # (|a| + |b| + 1) * 1001 >= 2^30
        Affine4Batch([(b"A", b"A"), (b"A" * 600000, b"A" * 600000)], AffineCost.double_affine(1000, 1, 1000, 1000, 1))
    with pytest.raises(ValueError):
        pa.align_affine4([(b"A", b"A")], AffineCost.affine(4, 6, 2))


def _create(cost, a=b"ACGT", b=b"ACGT"):
    L = capi.load()
    ap = (C.c_char_p * 1)(a)
    bp = (C.c_char_p * 1)(b)
    al, bl = np.array([len(a)], np.uint64), np.array([len(b)], np.uint64)
    sub, ins, dl, op, ex = cost
    c = capi._Affine4CostC(sub, ins, dl, (C.c_int32 * 4)(*op), (C.c_int32 * 4)(*ex))
    return L.pa_affine4_batch_create(ap, capi._p(al), bp, capi._p(bl), 1, C.byref(c), 0)


@pytest.mark.parametrize("cost", [
    (4, 0, 0, (0, 6, 24, 24), (2, 2, 1, 1)), (4, 0, 0, (6, 6, 24, 24), (2, 2, 1, 0)), (4, 0, 0, (6, 6, 0, 0), (2, 2, 0, 0)),
    (4, 0, 0, (6, 6, 24, 1001), (2, 2, 1, 1)), (4, 0, 0, (6, 6, 24, 24), (2, -1, 1, 1)), (-1, 0, 0, (6, 6, 24, 24), (2, 2, 1, 1)),
    (4, 1001, 0, (6, 6, 24, 24), (2, 2, 1, 1)), (4, 0, -3, (6, 6, 24, 24), (2, 2, 1, 1)),
])
def test_c_abi_rejects_cost_models(cost):
    assert not _create(cost)
    assert capi.last_error().startswith("pa_affine4_batch_create:")


def test_c_abi_rejects_null_model_and_overflow_sized_pairs():
    L = capi.load()
    assert not L.pa_affine4_batch_create(None, None, None, None, 0, None, 0)
    assert capi.last_error().startswith("pa_affine4_batch_create:")
    big = b"A" * 600000
    assert not _create((1000, 1000, 1000, (1, 1, 1, 1), (1000, 1, 1, 1)), big, big)
    msg = capi.last_error()
    assert msg.startswith("pa_affine4_batch_create:") and "pair 0" in msg and "2^30" in msg and "1001" in msg


def test_no_gpu_fails_loudly():
    if capi.load().pa_device_count() > 0:
        return
    with pytest.raises(pa.PaError):
        Affine4Batch([(b"ACGT", b"ACGT")], AffineCost.double_affine(4, 6, 2, 24, 1))
    with pytest.raises(pa.PaError):
        pa.align_affine4([(b"ACGT", b"AGGT")], AffineCost.double_affine(4, 6, 2, 24, 1))


def test_header_declares_what_capi_binds():
    txt = (ROOT / "include" / "pa_affine4_hip.h").read_text()
    body = re.search(r"typedef struct pa_affine4_cost\s*\{(.*?)\}\s*pa_affine4_cost;", txt, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["int32_t sub, ins, del", "int32_t open[4]", "int32_t extend[4]"]
    fields = capi._Affine4CostC._fields_
    assert [f for f, _ in fields] == ["sub", "ins", "del_", "open", "extend"]
    assert C.sizeof(capi._Affine4CostC) == 11 * 4 and C.sizeof(fields[3][1]) == 16 and C.sizeof(fields[4][1]) == 16
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert set(re.findall(r"\b(pa_affine4_[a-z_0-9]+)\s*\(", code)) == set(FUNCS)
    for fn in FUNCS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn)
    for word in ("ends-free", "chained strips", "tiled traceback", "diagonal-transition"):
        assert word in txt, word
    assert "pa_affine4_hip.h" in (ROOT / "include" / "pa_affine_hip.h").read_text()


def test_affine_batch_still_refuses_four_layers():
    with pytest.raises(ValueError):
        AffineCost.double_affine(4, 6, 2, 24, 1).to_c()
    with pytest.raises(ValueError):
        AffineBatch([(b"A", b"A")], AffineCost.double_affine(4, 6, 2, 24, 1))
    with pytest.raises(ValueError):
        pa.align_affine([(b"A", b"A")], AffineCost.double_affine(4, 6, 2, 24, 1))
