"""CPU-side checks of the chained gap-affine route: the header's declarations, the exported symbols, and the argument checks of the C ABI
and of align_affine that run before any device is touched."""
import re
from pathlib import Path

import pytest

import astar_pairwise_aligner_amd as pa
from astar_pairwise_aligner_amd import AffineCost, capi

ROOT = Path(__file__).resolve().parent.parent
PA_E_ARG = -4


def test_header_declares_the_chain_api():
    txt = (ROOT / "include" / "pa_affine_hip.h").read_text()
    for fn in ("pa_affine_batch_set_chain", "pa_affine_batch_chain_info"):
        assert re.search(r"\b" + fn + r"\(", txt), fn
        assert fn in capi.EXPORTED_SYMBOLS and hasattr(capi.load(), fn)
    assert re.search(r"int pa_affine_batch_set_chain\(pa_affine_batch\* ab, int on\);", txt)
    assert re.search(r"void pa_affine_batch_chain_info\(const pa_affine_batch\* ab, double\* on, double\* chain_pairs, double\* chain_jobs,"
                     r"\s*double\* chunks,\s*double\* bnd_bytes_max\);", txt)


def test_null_batch_is_an_argument_error():
    L = capi.load()
    assert L.pa_affine_batch_set_chain(None, 1) == PA_E_ARG
    assert capi.last_error().startswith("pa_affine_batch_set_chain:")


def test_chain_info_accepts_null_arguments():
    capi.load().pa_affine_batch_chain_info(None, None, None, None, None, None)


def test_align_affine_chain_needs_tiled():
    with pytest.raises(ValueError, match="tiled"):
        pa.align_affine([], AffineCost.affine(4, 6, 2), chain=True)
