"""CPU-side checks of the ends-free mode of the gap-affine batch: the header's declarations, the exported symbols, and the argument
checks of the C ABI, of AffineBatch and of map_affine that run before any device is touched."""
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineBatch, AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4
CM = AffineCost.affine(4, 6, 2)


def test_header_declares_the_ends_api():
    txt = (ROOT / "include" / "pa_affine_hip.h").read_text()
    for fn in ("pa_affine_batch_set_free_ends", "pa_affine_batch_ends", "pa_affine_batch_last_row"):
        assert re.search(r"\b" + fn + r"\(", txt), fn
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn)
    assert re.search(r"int pa_affine_batch_set_free_ends\(pa_affine_batch\* ab, int free_start, int free_end\);", txt)
    assert re.search(r"int pa_affine_batch_ends\(const pa_affine_batch\* ab, int64_t\* start_out, int64_t\* end_out\);", txt)
    assert re.search(r"int pa_affine_batch_last_row\(pa_affine_batch\* ab, int32_t\* out, const uint64_t\* offsets\);", txt)


@pytest.mark.parametrize("fn", ("pa_affine_batch_set_free_ends", "pa_affine_batch_ends", "pa_affine_batch_last_row"))
def test_null_batch_is_an_argument_error(fn):
    args = (None, 1, 1) if fn.endswith("free_ends") else (None, None, None)
    assert getattr(capi.load(), fn)(*args) == PA_E_ARG
    assert capi.last_error().startswith(fn + ":")


@pytest.mark.parametrize("bad", (2, -1, "yes", None, 1.0))
def test_bad_switch_values_raise_before_the_device_is_touched(bad):
    for kw in ({"free_start": bad}, {"free_end": bad}):
        with pytest.raises(ValueError, match="free_"):
            AffineBatch([(b"ACGT", b"ACG")], CM, **kw)
        with pytest.raises(ValueError, match="free_"):
            pa.map_affine([(b"ACGT", b"ACG")], CM, **kw)


def test_map_affine_chain_needs_tiled():
    with pytest.raises(ValueError, match="tiled"):
        pa.map_affine([], CM, chain=True)
    with pytest.raises(ValueError, match="tiled"):
        pa.align_affine([], CM, chain=True)
