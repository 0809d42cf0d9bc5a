"""CPU-side checks of the ends-free mode of the double-affine batch: the new header's declarations, the exported symbols, and the
argument checks of the C ABI, of Affine4Batch and of map_affine that run before any device is touched."""
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
CM = AffineCost.double_affine(4, 6, 2, 24, 1)
FUNCTIONS = ("pa_affine4_batch_set_free_ends", "pa_affine4_batch_ends", "pa_affine4_batch_last_row")


def test_header_declares_exactly_the_ends_api():
    txt = (ROOT / "include" / "pa_affine4_ends_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(re.findall(r"\b(pa_\w+)\(", code)) == sorted(FUNCTIONS)
    for fn in FUNCTIONS:
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn)
    assert re.search(r"int pa_affine4_batch_set_free_ends\(pa_affine4_batch\* ab, int free_start, int free_end\);", code)
    assert re.search(r"int pa_affine4_batch_ends\(const pa_affine4_batch\* ab, int64_t\* start_out, int64_t\* end_out\);", code)
    assert re.search(r"int pa_affine4_batch_last_row\(pa_affine4_batch\* ab, int32_t\* out, const uint64_t\* offsets\);", code)
    assert '#include "pa_affine4_hip.h"' in code
    main = (ROOT / "include" / "pa_affine4_hip.h").read_text()
    assert "pa_affine4_ends_hip.h" in main and not any(re.search(r"\b" + fn + r"\(", main) for fn in FUNCTIONS)
    assert re.search(r"Not supported:[^.]*diagonal-transition", main)  # still missing, and said so


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_null_batch_is_an_argument_error(fn):
    args = (None, 1, 1) if fn.endswith("free_ends") else (None, None, None)
    assert getattr(capi.load(), fn)(*args) == PA_E_ARG
    assert capi.last_error().startswith(fn + ":")


class _NoDevice(Affine4Batch):
    """An Affine4Batch without a handle: any call into the library would fail on it."""

    def __init__(self):
        self._h = None


@pytest.mark.parametrize("bad", (2, -1, "yes", None, 1.0))
def test_bad_switch_values_raise_before_the_device_is_touched(bad):
    for args in ((bad, True), (False, bad)):
        with pytest.raises(ValueError, match="free_"):
            _NoDevice().set_free_ends(*args)
    for kw in ({"free_start": bad}, {"free_end": bad}):
        with pytest.raises(ValueError, match="free_"):
            pa.map_affine([(b"ACGT", b"ACG")], CM, **kw)


def test_the_three_methods_are_the_base_class_s():
    for name in ("set_free_ends", "ends", "last_row"):
        assert getattr(Affine4Batch, name) is getattr(AffineBatch, name)
    assert Affine4Batch._PREFIX == "pa_affine4_batch" and AffineBatch._PREFIX == "pa_affine_batch"


def test_map_affine_has_no_diagonal_transition_for_four_layers():
    with pytest.raises(ValueError, match="diagonal transition has no double-affine route"):
        pa.map_affine([(b"ACGT", b"ACG")], CM, s_max=10)
    with pytest.raises(ValueError, match="diagonal transition has no double-affine route"):
        pa.map_affine([], CM, s_max=10, tiled=True)


def test_map_affine_chain_needs_tiled():
    with pytest.raises(ValueError, match="tiled"):
        pa.map_affine([], CM, chain=True)


def test_affine_batch_still_refuses_four_layers():
    with pytest.raises(ValueError, match="Affine4Batch"):
        AffineBatch([(b"ACGT", b"ACG")], CM)
