"""ctypes binding of libastarpa_c_hip.so -- exactly the symbols include/*.h declare.

There is no CPU fallback: if the library is missing or no GPU is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import _build

U64P = C.POINTER(C.c_uint64)

# every symbol include/astarpa.h and include/pa_bitpacking_hip.h declare
EXPORTED_SYMBOLS = [
    "astarpa2_simple", "astarpa2_full", "astarpa", "astarpa_gcsh", "astarpa_free_cigar",
    "pa_last_error", "pa_device_count", "pa_set_device",
    "pa_bp_profile_build", "pa_bp_compute", "pa_bp_fill", "pa_search", "pa_search_trace",
    "pa_batch_create", "pa_batch_run", "pa_batch_stats", "pa_batch_shape", "pa_batch_destroy",
    "pa_batch_create_banded", "pa_batch_create_trace", "pa_batch_align", "pa_batch_align_view", "pa_batch_trace_fallbacks", "pa_params_batch_align",
    "pa_pairs_read", "pa_pairs_count", "pa_pairs_get", "pa_pairs_free", "pa_write_results_csv", "pa_align_file",
    "pa_align", "pa_batch_align_multi", "pa_batch_create_trace_params",
    "pa_bp_ctx_create", "pa_bp_ctx_compute", "pa_bp_ctx_fill", "pa_bp_ctx_destroy",
    "pa_batch_create_params", "pa_batch_pair_stats", "pa_runtime_hints", "pa_batch_align_multi_params", "pa_release_pools", "pa_align_file_params", "pa_batch_params_supported", "pa_alloc_cache_stats", "pa_free_cigars",
    "pa_batch_full_info", "pa_batch_rdv_stats", "pa_combine_stats", "pa_params_nw", "pa_params_simple", "pa_params_full", "pa_debug_gcsh_probe", "pa_debug_gcsh_matches", "pa_debug_strip", "pa_batch_window_retries", "pa_batch_window_retry_bytes",
    "pa_batch_slice_info", "pa_set_reference_cost_only",
    "pa_search_batch_create", "pa_search_batch_run", "pa_search_batch_rows", "pa_search_batch_trace", "pa_search_batch_info",
    "pa_search_batch_destroy",
    "pa_affine_batch_create", "pa_affine_batch_run", "pa_affine_batch_align", "pa_affine_batch_info", "pa_affine_batch_destroy",
    "pa_affine_batch_align_tiled", "pa_affine_batch_tiled_info", "pa_affine_batch_set_chain", "pa_affine_batch_chain_info",
    "pa_affine_batch_set_free_ends", "pa_affine_batch_ends", "pa_affine_batch_last_row",
    "pa_affine_batch_run_dt", "pa_affine_batch_align_dt", "pa_affine_batch_dt_info",
    "pa_affine_batch_run_dt_ends", "pa_affine_batch_align_dt_ends",
    "pa_affine_batch_align_dt_seg", "pa_affine_batch_dt_seg_info",
    "pa_affine_batch_run_local", "pa_affine_batch_align_local", "pa_affine_batch_local_info",
    "pa_affine4_batch_create", "pa_affine4_batch_run", "pa_affine4_batch_align", "pa_affine4_batch_info", "pa_affine4_batch_destroy",
    "pa_affine4_batch_align_tiled", "pa_affine4_batch_tiled_info", "pa_affine4_batch_set_chain", "pa_affine4_batch_chain_info",
    "pa_affine4_batch_set_free_ends", "pa_affine4_batch_ends", "pa_affine4_batch_last_row",
    "pa_affine4_batch_run_dt", "pa_affine4_batch_align_dt", "pa_affine4_batch_run_dt_ends", "pa_affine4_batch_align_dt_ends",
    "pa_affine4_batch_dt_info",
    "pa_affine4_batch_align_dt_seg", "pa_affine4_batch_dt_seg_info",
    "pa_affine4_batch_run_local", "pa_affine4_batch_align_local", "pa_affine4_batch_local_info",
]

_lib = None


class PaError(RuntimeError):
    pass


def load(build_if_stale: bool = True) -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if os.environ.get("PA_LIB_PATH"):  # diagnostics: an alternative build of the same sources (e.g. -DPA_SWEEP_PHASE_TIMERS)
        from pathlib import Path

        path, build_if_stale = Path(os.environ["PA_LIB_PATH"]).resolve(), False
    if build_if_stale and _build.is_stale():
        try:
            _build.build()
        except Exception as e:  # stale but present is still usable on a box without hipcc
            if not path.exists():
                raise PaError(f"cannot build {path.name}: {e}") from e
    if not path.exists():
        raise PaError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    L = C.CDLL(str(path))
    L.pa_runtime_hints.restype = C.c_int
    if hasattr(L, "pa_set_reference_cost_only"):  # (PA_LIB_PATH may point at an older build of the library: diagnostics)
        L.pa_set_reference_cost_only.argtypes = [C.c_int]
        L.pa_set_reference_cost_only.restype = None
    L.pa_release_pools.restype = None
    L.pa_alloc_cache_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    L.pa_free_cigars.argtypes = [C.c_void_p, C.c_size_t]
    L.pa_free_cigars.restype = None
    L.pa_batch_params_supported.argtypes = [C.c_void_p]
    L.pa_batch_params_supported.restype = C.c_int
    L.pa_alloc_cache_stats.restype = None
    L.pa_runtime_hints()  # this package is the application here: more hardware queues, before the first HIP call
    vp, sz = C.c_void_p, C.c_size_t
    L.pa_last_error.restype = C.c_char_p
    L.pa_device_count.restype = C.c_int
    L.pa_set_device.argtypes = [C.c_int]
    L.pa_bp_profile_build.argtypes = [vp, sz, vp, sz, vp, vp]
    L.pa_bp_profile_build.restype = C.c_int
    L.pa_bp_compute.argtypes = [vp, sz, vp, sz, vp, vp, C.c_int]
    L.pa_bp_compute.restype = C.c_int32
    L.pa_bp_fill.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    L.pa_bp_fill.restype = C.c_int32
    L.pa_search.argtypes = [vp, sz, vp, sz, C.c_float, vp]
    L.pa_search.restype = C.c_int
    L.pa_search_trace.argtypes = [vp, sz, vp, sz, C.c_float, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz)]
    L.pa_search_trace.restype = C.c_int
    L.pa_search_batch_create.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp, sz, C.c_float]
    L.pa_search_batch_create.restype = vp
    L.pa_search_batch_run.argtypes = [vp, vp, vp, C.POINTER(C.c_float)]
    L.pa_search_batch_rows.argtypes = [vp, vp, vp]
    L.pa_search_batch_trace.argtypes = [vp, vp, vp, vp]
    L.pa_search_batch_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 4
    L.pa_search_batch_info.restype = None
    L.pa_search_batch_destroy.argtypes = [vp]
    L.pa_affine_batch_create.argtypes = [vp, vp, vp, vp, sz, vp, C.c_int]
    L.pa_affine_batch_create.restype = vp
    L.pa_affine_batch_run.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.pa_affine_batch_align.argtypes = [vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pa_affine_batch_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
    L.pa_affine_batch_info.restype = None
    L.pa_affine_batch_destroy.argtypes = [vp]
    if hasattr(L, "pa_affine_batch_align_tiled"):  # (PA_LIB_PATH may point at an older build of the library: diagnostics)
        L.pa_affine_batch_align_tiled.argtypes = [vp, C.c_uint32, vp, vp] + [C.POINTER(C.c_float)] * 3
        L.pa_affine_batch_tiled_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine_batch_tiled_info.restype = None
    if hasattr(L, "pa_affine_batch_set_chain"):
        L.pa_affine_batch_set_chain.argtypes = [vp, C.c_int]
        L.pa_affine_batch_chain_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine_batch_chain_info.restype = None
    if hasattr(L, "pa_affine_batch_set_free_ends"):
        L.pa_affine_batch_set_free_ends.argtypes = [vp, C.c_int, C.c_int]
        L.pa_affine_batch_ends.argtypes = [vp, vp, vp]
        L.pa_affine_batch_last_row.argtypes = [vp, vp, vp]
    if hasattr(L, "pa_affine_batch_run_dt"):
        L.pa_affine_batch_run_dt.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_float)]
        L.pa_affine_batch_align_dt.argtypes = [vp, C.c_int32, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pa_affine_batch_dt_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 6
        L.pa_affine_batch_dt_info.restype = None
    if hasattr(L, "pa_affine_batch_run_dt_ends"):
        L.pa_affine_batch_run_dt_ends.argtypes = [vp, C.c_int, C.c_int, C.c_int32, vp, vp, C.POINTER(C.c_float)]
        L.pa_affine_batch_align_dt_ends.argtypes = [vp, C.c_int, C.c_int, C.c_int32, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(L, "pa_affine_batch_align_dt_seg"):
        L.pa_affine_batch_align_dt_seg.argtypes = [vp, C.c_int, C.c_int, C.c_int32, C.c_uint32, vp, vp, vp, vp] + [C.POINTER(C.c_float)] * 3
        L.pa_affine_batch_dt_seg_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine_batch_dt_seg_info.restype = None
    if hasattr(L, "pa_affine_batch_run_local"):
        L.pa_affine_batch_run_local.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(C.c_float)]
        L.pa_affine_batch_align_local.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pa_affine_batch_local_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 2
        L.pa_affine_batch_local_info.restype = None
    if hasattr(L, "pa_affine4_batch_create"):
        L.pa_affine4_batch_create.argtypes = [vp, vp, vp, vp, sz, vp, C.c_int]
        L.pa_affine4_batch_create.restype = vp
        L.pa_affine4_batch_run.argtypes = [vp, vp, C.POINTER(C.c_float)]
        L.pa_affine4_batch_align.argtypes = [vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pa_affine4_batch_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine4_batch_info.restype = None
        L.pa_affine4_batch_destroy.argtypes = [vp]
        L.pa_affine4_batch_destroy.restype = None
    if hasattr(L, "pa_affine4_batch_align_tiled"):
        L.pa_affine4_batch_align_tiled.argtypes = [vp, C.c_uint32, vp, vp] + [C.POINTER(C.c_float)] * 3
        L.pa_affine4_batch_tiled_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine4_batch_tiled_info.restype = None
    if hasattr(L, "pa_affine4_batch_set_chain"):
        L.pa_affine4_batch_set_chain.argtypes = [vp, C.c_int]
        L.pa_affine4_batch_chain_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine4_batch_chain_info.restype = None
    if hasattr(L, "pa_affine4_batch_set_free_ends"):
        L.pa_affine4_batch_set_free_ends.argtypes = [vp, C.c_int, C.c_int]
        L.pa_affine4_batch_ends.argtypes = [vp, vp, vp]
        L.pa_affine4_batch_last_row.argtypes = [vp, vp, vp]
    if hasattr(L, "pa_affine4_batch_run_dt"):
        L.pa_affine4_batch_run_dt.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_float)]
        L.pa_affine4_batch_align_dt.argtypes = [vp, C.c_int32, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pa_affine4_batch_run_dt_ends.argtypes = [vp, C.c_int, C.c_int, C.c_int32, vp, vp, C.POINTER(C.c_float)]
        L.pa_affine4_batch_align_dt_ends.argtypes = [vp, C.c_int, C.c_int, C.c_int32, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pa_affine4_batch_dt_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 6
        L.pa_affine4_batch_dt_info.restype = None
    if hasattr(L, "pa_affine4_batch_align_dt_seg"):
        L.pa_affine4_batch_align_dt_seg.argtypes = [vp, C.c_int, C.c_int, C.c_int32, C.c_uint32, vp, vp, vp, vp] + [C.POINTER(C.c_float)] * 3
        L.pa_affine4_batch_dt_seg_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
        L.pa_affine4_batch_dt_seg_info.restype = None
    if hasattr(L, "pa_affine4_batch_run_local"):
        L.pa_affine4_batch_run_local.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(C.c_float)]
        L.pa_affine4_batch_align_local.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pa_affine4_batch_local_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 2
        L.pa_affine4_batch_local_info.restype = None
    L.pa_search_batch_destroy.restype = None
    L.pa_batch_create.argtypes = [vp, vp, vp, vp, sz]
    L.pa_batch_create.restype = vp
    L.pa_batch_run.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.pa_batch_run.restype = C.c_int
    L.pa_batch_stats.argtypes = [vp] + [C.POINTER(C.c_double)] * 4
    L.pa_batch_full_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_double)]
    L.pa_batch_full_info.restype = None
    L.pa_batch_rdv_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.pa_combine_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pa_combine_stats.restype = None
    L.pa_batch_rdv_stats.restype = C.c_int
    L.pa_batch_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.pa_batch_slice_info.argtypes = [vp] + [C.POINTER(C.c_double)] * 5
    L.pa_batch_slice_info.restype = C.c_int
    L.pa_batch_destroy.argtypes = [vp]
    L.pa_batch_create_banded.argtypes = [vp, vp, vp, vp, sz, C.c_float]
    L.pa_batch_create_banded.restype = vp
    L.pa_batch_create_trace.argtypes = [vp, vp, vp, vp, sz]
    L.pa_batch_create_trace.restype = vp
    L.pa_bp_ctx_create.argtypes = [vp, sz, vp, sz]
    L.pa_bp_ctx_create.restype = vp
    L.pa_bp_ctx_compute.argtypes = [vp, C.c_int32, C.c_int32, sz, sz, vp, C.c_int, C.POINTER(C.c_int32)]
    L.pa_bp_ctx_compute.restype = C.c_int
    L.pa_bp_ctx_fill.argtypes = [vp, C.c_int32, C.c_int32, sz, sz, vp, vp, vp]
    L.pa_bp_ctx_fill.restype = C.c_int
    L.pa_bp_ctx_destroy.argtypes = [vp]
    L.pa_batch_create_trace_params.argtypes = [vp, vp, vp, vp, sz, vp]
    L.pa_batch_create_trace_params.restype = vp
    L.pa_batch_create_params.argtypes = [vp, vp, vp, vp, sz, vp]
    L.pa_batch_create_params.restype = vp
    L.pa_batch_pair_stats.argtypes = [vp, vp]
    L.pa_batch_pair_stats.restype = C.c_int
    L.pa_batch_align.argtypes = [vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pa_batch_align.restype = C.c_int
    L.pa_batch_align_view.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pa_batch_align_view.restype = C.c_int
    L.pa_batch_trace_fallbacks.argtypes = [vp]
    L.pa_batch_trace_fallbacks.restype = C.c_size_t
    L.pa_batch_window_retries.argtypes = [vp]
    L.pa_batch_window_retries.restype = C.c_size_t
    L.pa_pairs_read.argtypes = [C.c_char_p]
    L.pa_pairs_read.restype = vp
    L.pa_pairs_count.argtypes = [vp]
    L.pa_pairs_count.restype = sz
    L.pa_pairs_get.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
    L.pa_pairs_get.restype = C.c_int
    L.pa_pairs_free.argtypes = [vp]
    L.pa_write_results_csv.argtypes = [C.c_char_p, vp, vp, sz]
    L.pa_write_results_csv.restype = C.c_int
    L.pa_batch_align_multi.argtypes = [vp, vp, vp, vp, sz, C.POINTER(C.c_int), C.c_int, vp, vp]
    L.pa_batch_align_multi.restype = C.c_int
    L.pa_batch_align_multi_params.argtypes = [vp, vp, vp, vp, sz, C.POINTER(C.c_int), C.c_int, vp, vp, vp, vp]
    L.pa_batch_align_multi_params.restype = C.c_int
    L.pa_align_file.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(sz)]
    L.pa_align_file.restype = C.c_int
    L.pa_align_file_params.argtypes = [C.c_char_p, C.c_char_p, vp, C.POINTER(sz)]
    L.pa_align_file_params.restype = C.c_int
    for name in ("astarpa2_simple", "astarpa2_full", "astarpa"):
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes = [vp, sz, vp, sz, C.POINTER(vp), C.POINTER(sz)]
            f.restype = C.c_uint64
    if hasattr(L, "astarpa_gcsh"):
        L.astarpa_gcsh.argtypes = [vp, sz, vp, sz, sz, sz, C.c_bool, C.POINTER(vp), C.POINTER(sz)]
        L.astarpa_gcsh.restype = C.c_uint64
    if hasattr(L, "astarpa_free_cigar"):
        L.astarpa_free_cigar.argtypes = [vp]
    _lib = L
    return L


def last_error() -> str:
    return (load().pa_last_error() or b"").decode()


def _p(arr: np.ndarray):
    return arr.ctypes.data_as(C.c_void_p)


def _buf(b: bytes):
    return C.cast(C.c_char_p(b), C.c_void_p)


def _marshal_pairs(pairs):
    """(a pointers, a lengths, b pointers, b lengths) for the `const uint8_t* const*` / `const size_t*` arguments.  c_char_p arrays
    point straight into the bytes objects (the caller keeps `pairs` alive); building them is 40x cheaper than one ctypes cast per
    sequence, which used to cost more than the GPU work of a 10 000-pair batch."""
    n = len(pairs)
    if any(not isinstance(a, bytes) or not isinstance(b, bytes) for a, b in pairs):
        raise ValueError("pairs must be (bytes, bytes) tuples")
    ap = (C.c_char_p * max(n, 1))(*[a for a, _ in pairs])
    bp = (C.c_char_p * max(n, 1))(*[b for _, b in pairs])
    al = np.fromiter((len(a) for a, _ in pairs), dtype=np.uint64, count=n) if n else np.zeros(1, np.uint64)
    bl = np.fromiter((len(b) for _, b in pairs), dtype=np.uint64, count=n) if n else np.zeros(1, np.uint64)
    return ap, _p(al), bp, _p(bl)


def alloc_cache_stats() -> dict:
    """pa_alloc_cache_stats: the library's cache of large device buffers (pa_astarpa2.h)."""
    h, m, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    load().pa_alloc_cache_stats(C.byref(h), C.byref(m), C.byref(b))
    return {"hits": h.value, "misses": m.value, "cached_bytes": b.value}


def batch_params_supported(params) -> bool:
    """pa_batch_params_supported: does pa_batch_create_params take this AstarPa2Params (Domain::Astar over sparse 256-column blocks with a
    search: the `simple` and `full` presets and their relatives)?"""
    cp = params._to_c()
    return load().pa_batch_params_supported(C.byref(cp)) == 1


def gcsh_probe(a: bytes, b: bytes, k: int, p: int, queries) -> tuple[list[int], int]:
    """pa_debug_gcsh_probe (diagnostics): GCSH h at `queries` [(i, j), ..] as the GPU computes it -- contours derived and probed by one
    wavefront (csrc/apa2_full_kernel.hpp) -- and the number of contour layers."""
    L = load()
    L.pa_debug_gcsh_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pa_debug_gcsh_probe.restype = C.c_int
    q = np.ascontiguousarray(np.array(queries, np.int32).reshape(-1, 2))
    out = np.zeros(len(q) + 1, np.int32)
    rc = L.pa_debug_gcsh_probe(_buf(a), len(a), _buf(b), len(b), k, p, _p(q), len(q), _p(out))
    if rc != 0:
        raise PaError(f"pa_debug_gcsh_probe rc={rc}: {last_error()}")
    return out[:-1].tolist(), int(out[-1])


def gcsh_matches(a: bytes, b: bytes, k: int, p: int) -> list[tuple[int, int]]:
    """pa_debug_gcsh_matches (diagnostics): the matches GCSH keeps for this pair as the GPU finds them (csrc/gcsh_build_kernel.hpp), by start."""
    L = load()
    L.pa_debug_gcsh_matches.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
    L.pa_debug_gcsh_matches.restype = C.c_long
    cap = len(a) // max(1, k) * 2 + 4096
    out = np.zeros((cap, 2), np.int32)
    n = L.pa_debug_gcsh_matches(_buf(a), len(a), _buf(b), len(b), k, p, _p(out), cap)
    if n < 0:
        raise PaError(f"pa_debug_gcsh_matches rc={n}: {last_error()}")
    return [tuple(x) for x in out[:n].tolist()]


class _StripProbeJob(C.Structure):
    _fields_ = [("a", C.c_void_p), ("a_len", C.c_size_t), ("b", C.c_void_p), ("b_len", C.c_size_t)] + [
        (f, C.c_int32) for f in ("col0", "n", "word0", "nlanes", "tap", "fill_word0", "fill_stride", "hin_is_hout")
    ] + [("v", C.c_void_p), ("hin", C.c_void_p), ("values", C.c_void_p), ("hout", C.c_void_p), ("sum", C.c_int32)]


STRIP_DUAL, STRIP_SINGLE, STRIP_RDV = 0, 1, 2


def strip_probe(mode: int, variant: int, jobs, nwaves: int = 0, patience: int = 0):
    """pa_debug_strip (tests): strip jobs of the batched A*PA2 band search through the strips those kernels run (csrc/strip2_kernel.hpp,
    csrc/strip_kernel.hpp).  `jobs`: dicts with a, b (ACGT bytes), col0, n, word0, nlanes, v (uint64 [ceil(|b| / 64), 2]: V(p, m) per
    word), hout (uint8 [|a|]) and optionally hin (uint8 [|a|]), hin_is_hout, tap, values (like v), fill_word0, fill_stride.  Inputs are
    not modified.  Returns ([{"v", "hout", "sum"} per job], rendezvous counters (took, served, alone, withdrawn) or None)."""
    L = load()
    L.pa_debug_strip.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pa_debug_strip.restype = C.c_int
    arr = (_StripProbeJob * max(len(jobs), 1))()
    keep = []
    outs = []
    for t, jd in enumerate(jobs):
        a, b = bytes(jd["a"]), bytes(jd["b"])
        v = np.array(jd["v"], np.uint64, copy=True, order="C")
        hout = np.array(jd["hout"], np.uint8, copy=True, order="C")
        hin = None if jd.get("hin") is None else np.ascontiguousarray(jd["hin"], np.uint8)
        values = None if jd.get("values") is None else np.ascontiguousarray(jd["values"], np.uint64)
        keep += [a, b, hin, values]
        x = arr[t]
        x.a, x.a_len, x.b, x.b_len = _buf(a).value, len(a), _buf(b).value, len(b)
        x.col0, x.n, x.word0, x.nlanes = jd["col0"], jd["n"], jd["word0"], jd["nlanes"]
        x.tap, x.fill_word0, x.fill_stride, x.hin_is_hout = jd.get("tap", -1), jd.get("fill_word0", 0), jd.get("fill_stride", 0), int(jd.get("hin_is_hout", 0))
        x.v, x.hout = v.ctypes.data, hout.ctypes.data
        x.hin = None if hin is None else hin.ctypes.data
        x.values = None if values is None else values.ctypes.data
        outs.append({"v": v, "hout": hout})
    cnt = np.zeros(4, np.uint64)
    rc = L.pa_debug_strip(mode, variant, nwaves, patience, C.cast(arr, C.c_void_p) if jobs else None, len(jobs), _p(cnt))
    if rc != 0:
        raise PaError(f"pa_debug_strip rc={rc}: {last_error()}")
    for t, o in enumerate(outs):
        o["sum"] = int(arr[t].sum)
    return outs, (tuple(int(c) for c in cnt) if mode == STRIP_RDV else None)


def release_pools() -> None:
    """pa_release_pools: the calling thread's engine pools and the cache of large device buffers back to the driver."""
    load().pa_release_pools()


def require_gpu() -> None:
    if load().pa_device_count() <= 0:
        raise PaError("no MI355X visible: the HIP path is required (no CPU fallback)")


def profile_build(a: bytes, b: bytes):
    """BitProfile::build on the GPU -> (a2[n,2], b2[w,2]) uint64."""
    L = load()
    a2 = np.zeros((len(a), 2), np.uint64)
    b2 = np.zeros(((len(b) + 63) // 64, 2), np.uint64)
    rc = L.pa_bp_profile_build(_buf(a), len(a), _buf(b), len(b), _p(a2), _p(b2))
    if rc == -1:
        raise ValueError("sequence contains a character outside ACGT")
    if rc != 0:
        raise PaError(last_error())
    return a2, b2


def compute(a2, b2, h2, v2, exact_end: bool) -> int:
    r = load().pa_bp_compute(_p(a2), len(a2), _p(b2), len(b2), _p(h2), _p(v2), int(exact_end))
    if r == -(2 ** 31):
        raise PaError(last_error())
    return r


def fill(a2, b2, h2, v2):
    values = np.zeros((len(a2), len(b2), 2), np.uint64)
    r = load().pa_bp_fill(_p(a2), len(a2), _p(b2), len(b2), _p(h2), _p(v2), _p(values))
    if r == -(2 ** 31):
        raise PaError(last_error())
    return r, values


def search(pattern: bytes, text: bytes, unmatched_cost: float) -> list[int]:
    """pa_bitpacking::search(pattern, text, unmatched_cost).out on the GPU (search.rs:46-120)."""
    out = np.zeros(len(pattern) + len(text) + 1, np.int32)
    rc = load().pa_search(_buf(pattern), len(pattern), _buf(text), len(text), unmatched_cost, _p(out))
    if rc == -1:
        raise ValueError("unknown base")
    if rc != 0:
        raise PaError(f"pa_search rc={rc}: {last_error()}")
    return out.tolist()


def search_trace(pattern: bytes, text: bytes, unmatched_cost: float, idx: int):
    """SearchResult::trace(idx) (search.rs:125-228) -> (CIGAR string, [(text index, pattern index), ...])."""
    L = load()
    cig, path, npos = C.c_void_p(None), C.c_void_p(None), C.c_size_t(0)
    rc = L.pa_search_trace(_buf(pattern), len(pattern), _buf(text), len(text), unmatched_cost, idx, C.byref(cig), C.byref(path),
                           C.byref(npos))
    try:
        if rc == -1:
            raise ValueError("unknown base")
        if rc != 0:
            raise PaError(f"pa_search_trace rc={rc}: {last_error()}")
        text_cigar = C.string_at(cig.value).decode()
        arr = np.ctypeslib.as_array(C.cast(path.value, C.POINTER(C.c_int32)), shape=(2 * npos.value,)).copy() if npos.value else np.zeros(0, np.int32)
    finally:
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        if cig.value:
            libc.free(cig)
        if path.value:
            libc.free(path)
    return text_cigar, [(int(arr[2 * k]), int(arr[2 * k + 1])) for k in range(npos.value)]


class SearchBatch:
    """Many semi-global searches in one pass (pa_search_batch_*): query q searches patterns[i] in texts[j] for queries[q] = (i, j).
    Every pattern and text is uploaded once, however many queries use it."""

    def __init__(self, patterns: list[bytes], texts: list[bytes], queries, unmatched_cost: float):
        L = load()
        if any(not isinstance(x, bytes) for x in list(patterns) + list(texts)):
            raise ValueError("patterns and texts must be bytes")
        q = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
        if q.size and (q.min() < 0 or q[:, 0].max() >= len(patterns) or q[:, 1].max() >= len(texts)):
            raise ValueError("query index out of range")
        self._keep = (list(patterns), list(texts))
        self.plens = np.array([len(p) for p in patterns] or [0], np.uint64)
        self.tlens = np.array([len(t) for t in texts] or [0], np.uint64)
        self.q_pattern = np.ascontiguousarray(q[:, 0], np.uint32) if len(q) else np.zeros(1, np.uint32)
        self.q_text = np.ascontiguousarray(q[:, 1], np.uint32) if len(q) else np.zeros(1, np.uint32)
        self.queries = len(q)
        pp = (C.c_char_p * max(len(patterns), 1))(*patterns)
        tp = (C.c_char_p * max(len(texts), 1))(*texts)
        self._h = L.pa_search_batch_create(pp, _p(self.plens), len(patterns), tp, _p(self.tlens), len(texts), _p(self.q_pattern),
                                           _p(self.q_text), self.queries, C.c_float(unmatched_cost))
        if not self._h:
            msg = last_error()
            if "unknown base" in msg or "actgACTG" in msg:
                raise ValueError(msg)
            raise PaError(msg)
        self.last_kernel_ms = 0.0

    def _check(self, rc: int, what: str) -> None:
        if rc == -1:
            raise ValueError(last_error())
        if rc != 0:
            raise PaError(f"{what} rc={rc}: {last_error()}")

    def _lens(self, q: int) -> int:
        return int(self.plens[self.q_pattern[q]]) + int(self.tlens[self.q_text[q]]) + 1

    def run(self):
        """-> (best cost int32[queries], lowest index reaching it uint64[queries]); the kernel time is kept in `last_kernel_ms`."""
        costs = np.zeros(max(self.queries, 1), np.int32)
        idx = np.zeros(max(self.queries, 1), np.uint64)
        ms = C.c_float(0)
        self._check(load().pa_search_batch_run(self._h, _p(costs), _p(idx), C.byref(ms)), "pa_search_batch_run")
        self.last_kernel_ms = float(ms.value)
        return costs[: self.queries], idx[: self.queries]

    def rows(self, queries=None) -> list[np.ndarray]:
        """pa_search's out array of every query (or of the listed ones), after run()."""
        sel = range(self.queries) if queries is None else [int(q) for q in queries]
        offsets = np.full(max(self.queries, 1), np.iinfo(np.uint64).max, np.uint64)
        total = 0
        for q in sel:
            offsets[q] = total
            total += self._lens(q)
        out = np.zeros(max(total, 1), np.int32)
        self._check(load().pa_search_batch_rows(self._h, _p(out), _p(offsets)), "pa_search_batch_rows")
        return [out[int(offsets[q]): int(offsets[q]) + self._lens(q)] for q in sel]

    def trace(self, idx=None) -> list[tuple[str, tuple[int, int]]]:
        """[(CIGAR, (text index, pattern index) where the alignment starts)] of every query's best hit, or of idx[q]."""
        L = load()
        n = self.queries
        cig = (C.c_void_p * max(n, 1))()
        starts = np.zeros(2 * max(n, 1), np.int64)
        want = None
        if idx is not None:
            want = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
            if len(want) != n:
                raise ValueError("one index per query")
        rc = L.pa_search_batch_trace(self._h, _p(want) if want is not None else None, cig, _p(starts))
        try:
            self._check(rc, "pa_search_batch_trace")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        return [(cigars[q], (int(starts[2 * q]), int(starts[2 * q + 1]))) for q in range(n)]

    def info(self) -> dict:
        vals = [C.c_double(0) for _ in range(4)]
        load().pa_search_batch_info(self._h, *[C.byref(v) for v in vals])
        return {"waves": int(vals[0].value), "packed": int(vals[1].value), "chained": int(vals[2].value), "lane_use": vals[3].value}

    def close(self):
        if self._h:
            load().pa_search_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _AffineCostC(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("sub", "ins", "del_", "ins_open", "ins_extend", "del_open", "del_extend")]


class _Affine4CostC(C.Structure):
    _fields_ = [("sub", C.c_int32), ("ins", C.c_int32), ("del_", C.c_int32), ("open", C.c_int32 * 4), ("extend", C.c_int32 * 4)]


AFFINE_MAX_COST = 1000
AFFINE_ROWS_PER_LANE = 16  # rows of b per lane of the kernel (csrc/affine_kernel.hpp kRows)
AFFINE4_ROWS_PER_LANE = 16  # ... of the double-affine kernel (csrc/affine4_kernel.hpp kRows)
AFFINE4_LAYER_KINDS = ["ins", "del", "ins", "del"]


class AffineCost:
    """A gap-affine cost model: AffineCost<0> or AffineCost<2> of pa-affine-types (cost_model.rs:112-190).  None = no such edge.
    `layers` lists the affine layers as (kind, open, extend), kind "ins" or "del", in the reference's order [insert, delete]; a gap of
    length L in a layer costs open + L * extend."""

    def __init__(self, sub=None, ins=None, del_=None, layers=()):
        self.sub, self.ins, self.del_ = sub, ins, del_
        self.layers = [tuple(x) for x in layers]

    @classmethod
    def lcs(cls):
        return cls(None, 1, 1)

    @classmethod
    def unit(cls):
        return cls(1, 1, 1)

    @classmethod
    def linear(cls, sub, indel):
        return cls(sub, indel, indel)

    @classmethod
    def linear_asymmetric(cls, sub, ins, del_):
        return cls(sub, ins, del_)

    @classmethod
    def affine(cls, sub, open, extend):
        return cls(sub, None, None, [("ins", open, extend), ("del", open, extend)])

    @classmethod
    def linear_affine(cls, sub, indel, open, extend):
        return cls(sub, indel, indel, [("ins", open, extend), ("del", open, extend)])

    @classmethod
    def affine_asymmetric(cls, sub, ins_open, ins_extend, del_open, del_extend):
        return cls(sub, None, None, [("ins", ins_open, ins_extend), ("del", del_open, del_extend)])

    @classmethod
    def double_affine(cls, sub, open, extend, open2, extend2):
        """AffineCost<4>, the two-piece gap cost: a gap of length L costs min(open + L extend, open2 + L extend2).  Affine4Batch and
        align_affine4 run it (to_c4); AffineBatch, whose kernels have two layers, refuses it."""
        return cls(sub, None, None, [("ins", open, extend), ("del", open, extend), ("ins", open2, extend2), ("del", open2, extend2)])

    def ins_layer(self):
        return next(((o, e) for k, o, e in self.layers if k == "ins"), None)

    def del_layer(self):
        return next(((o, e) for k, o, e in self.layers if k == "del"), None)

    def to_c(self) -> _AffineCostC:
        """The pa_affine_cost of this model; ValueError for what the GPU kernel does not take."""
        if len(self.layers) > 2 or [k for k, _, _ in self.layers] not in ([], ["ins", "del"]):
            raise ValueError(f"only AffineCost<0> and AffineCost<2> with layers [ins, del] are supported, got {self.layers}"
                             " (Affine4Batch takes the four layers [ins, del, ins, del])")
        vals = [self.sub, self.ins, self.del_] + [x for _, o, e in self.layers for x in (o, e)]
        for v in vals:
            if v is not None and (not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= AFFINE_MAX_COST):
                raise ValueError(f"every cost must be an integer in [1, {AFFINE_MAX_COST}], got {v!r}")
        il, dl = self.ins_layer(), self.del_layer()
        if self.ins is None and il is None:
            raise ValueError("the cost model has no insertion edge")
        if self.del_ is None and dl is None:
            raise ValueError("the cost model has no deletion edge")
        z = lambda v: 0 if v is None else int(v)  # noqa: E731
        return _AffineCostC(z(self.sub), z(self.ins), z(self.del_), z(il and il[0]), z(il and il[1]), z(dl and dl[0]), z(dl and dl[1]))

    def to_c4(self) -> _Affine4CostC:
        """The pa_affine4_cost of this model: exactly the four layers [ins, del, ins, del]; ValueError for anything else, and for a
        cost that is not an integer in [1, 1000]."""
        if [k for k, _, _ in self.layers] != AFFINE4_LAYER_KINDS:
            raise ValueError(f"only AffineCost<4> with layers [ins, del, ins, del] is supported, got {self.layers}")
        vals = [self.sub, self.ins, self.del_] + [x for _, o, e in self.layers for x in (o, e)]
        for v in vals:
            if v is not None and (not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= AFFINE_MAX_COST):
                raise ValueError(f"every cost must be an integer in [1, {AFFINE_MAX_COST}], got {v!r}")
        if any(o is None or e is None for _, o, e in self.layers):
            raise ValueError("every layer needs both open and extend")
        z = lambda v: 0 if v is None else int(v)  # noqa: E731
        return _Affine4CostC(z(self.sub), z(self.ins), z(self.del_), (C.c_int32 * 4)(*[int(o) for _, o, _ in self.layers]),
                             (C.c_int32 * 4)(*[int(e) for _, _, e in self.layers]))

    def max_edge(self) -> int:
        return max([v for v in (self.sub, self.ins, self.del_) if v is not None] + [o + e for _, o, e in self.layers])

    def __repr__(self):
        return f"AffineCost(sub={self.sub}, ins={self.ins}, del_={self.del_}, layers={self.layers})"


def _switch(v, name: str) -> int:
    """A free_start / free_end value: a bool, or the integer 0 or 1."""
    if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and int(v) in (0, 1)):
        return int(v)
    raise ValueError(f"{name} must be a bool (or 0 / 1), got {v!r}")


AFFINE_MAX_MATCH = 1000


def _match_arg(match) -> int:
    """The bonus per match of a local-alignment call: an integer in [1, 1000]."""
    if not isinstance(match, (int, np.integer)) or isinstance(match, (bool, np.bool_)) or not 1 <= match <= AFFINE_MAX_MATCH:
        raise ValueError(f"match must be an integer in [1, {AFFINE_MAX_MATCH}], got {match!r}")
    return int(match)


def _s_max_arg(s_max) -> int:
    """The bound of a diagonal-transition call: an integer in [0, 2^30)."""
    if not isinstance(s_max, (int, np.integer)) or isinstance(s_max, bool) or not 0 <= s_max < 1 << 30:
        raise ValueError(f"s_max must be an integer in [0, 2^30), got {s_max!r}")
    return int(s_max)


class _AffineBatchBase:
    """What AffineBatch (pa_affine_batch_*) and Affine4Batch (pa_affine4_batch_*) share: the C functions of either differ in their
    prefix, `_PREFIX`, in the cost structure they take, `_cost_c`, and in where align_tiled() keeps the walk time, `_WALK_MS`.  Both have
    the chained route (set_chain, chain_info), ends-free mode (set_free_ends, ends, last_row) and the diagonal-transition route (run_dt,
    align_dt, run_dt_ends, align_dt_ends, dt_info)."""

    _PREFIX = ""
    _WALK_MS = "last_trace_ms"

    @staticmethod
    def _cost_c(cm: AffineCost):
        raise NotImplementedError

    def _fn(self, name: str):
        return getattr(load(), f"{self._PREFIX}_{name}")

    def __init__(self, pairs, cm: AffineCost, trace: bool = False):
        pairs = list(pairs)
        if any(not isinstance(x, bytes) or not isinstance(y, bytes) for x, y in pairs):
            raise ValueError("pairs must be (bytes, bytes)")
        if not isinstance(cm, AffineCost):
            raise ValueError("cm must be an AffineCost")
        c = self._cost_c(cm)
        big = cm.max_edge()
        for p, (x, y) in enumerate(pairs):
            if (len(x) + len(y) + 1) * big >= 1 << 30:
                raise ValueError(f"pair {p}: (|a| + |b| + 1) * max edge cost is not below 2^30")
        self._keep = pairs
        self.npairs = len(pairs)
        self.trace = bool(trace)
        n = max(len(pairs), 1)
        ap = (C.c_char_p * n)(*[x for x, _ in pairs])
        bp = (C.c_char_p * n)(*[y for _, y in pairs])
        al = np.array([len(x) for x, _ in pairs] or [0], np.uint64)
        bl = np.array([len(y) for _, y in pairs] or [0], np.uint64)
        self._c = c
        self._h = self._fn("create")(ap, _p(al), bp, _p(bl), len(pairs), C.byref(c), int(self.trace))
        if not self._h:
            msg = last_error()
            if msg.startswith(f"{self._PREFIX}_create:"):
                raise ValueError(msg)
            raise PaError(msg)
        self.last_kernel_ms = 0.0
        self.last_forward_ms = 0.0
        self.last_refill_ms = 0.0
        self.last_trace_ms = 0.0

    def _check(self, rc: int, what: str) -> None:
        if rc == -4:
            raise ValueError(last_error())
        if rc != 0:
            raise PaError(f"{what} rc={rc}: {last_error()}")

    def run(self) -> np.ndarray:
        """Costs only: int32[npairs]; the kernel time is kept in `last_kernel_ms`.  May be called again."""
        costs = np.zeros(max(self.npairs, 1), np.int32)
        ms = C.c_float(0)
        self._check(self._fn("run")(self._h, _p(costs), C.byref(ms)), f"{self._PREFIX}_run")
        self.last_kernel_ms = float(ms.value)
        return costs[: self.npairs]

    def _traced(self, name: str, args: tuple, times: tuple) -> list[tuple[int, str]]:
        """[(cost, CIGAR)] of every pair from the C function `name`, which takes `args`, the outputs and one float per attribute of
        `times`."""
        n = self.npairs
        costs = np.zeros(max(n, 1), np.int32)
        cig = (C.c_void_p * max(n, 1))()
        ms = [C.c_float(0) for _ in times]
        rc = self._fn(name)(self._h, *args, _p(costs), cig, *[C.byref(t) for t in ms])
        try:
            self._check(rc, f"{self._PREFIX}_{name}")
            cigars = _c_strings(cig, n)
        finally:
            load().pa_free_cigars(cig, n)
        for attr, t in zip(times, ms):
            setattr(self, attr, float(t.value))
        return [(int(costs[p]), cigars[p]) for p in range(n)]

    def align(self) -> list[tuple[int, str]]:
        """[(cost, CIGAR)] of every pair (trace batches only), in chunks whose traceback codes stay within PA_AFFINE_TRACE_BUDGET_MB;
        ValueError naming a pair whose codes alone exceed it."""
        return self._traced("align", (), ("last_forward_ms", "last_trace_ms"))

    def align_tiled(self, tile_cols: int = 0) -> list[tuple[int, str]]:
        """align() in bounded device memory: checkpoints from a cost-only pass, then only the tiles the path crosses are filled with
        codes and walked.  tile_cols: columns of a tile, 0 for the default of 1024, else in [64, 2^20].  The times are kept in
        `last_forward_ms` (checkpoint pass), `last_refill_ms` (tile fills) and the walks' in `last_trace_ms` (AffineBatch) or
        `last_walk_ms` (Affine4Batch)."""
        if not isinstance(tile_cols, (int, np.integer)) or isinstance(tile_cols, bool) or not 0 <= tile_cols < 1 << 32:
            raise ValueError(f"tile_cols must be 0 or in [64, 2^20], got {tile_cols!r}")
        return self._traced("align_tiled", (int(tile_cols),), ("last_forward_ms", "last_refill_ms", self._WALK_MS))

    def tiled_info(self) -> dict:
        """Shape of the last align_tiled(): chunks, rounds, tile jobs, cells the fills computed, bytes of the largest chunk."""
        vals = [C.c_double(0) for _ in range(5)]
        self._fn("tiled_info")(self._h, *[C.byref(v) for v in vals])
        return {k: int(v.value) for k, v in zip(("chunks", "rounds", "tile_jobs", "refill_cells", "chunk_bytes_max"), vals)}

    def info(self) -> dict:
        """The plan of run(): waves, packed and strip pairs, the share of lanes that hold rows; and the chunks of the last align()."""
        vals = [C.c_double(0) for _ in range(5)]
        self._fn("info")(self._h, *[C.byref(v) for v in vals])
        return {"waves": int(vals[0].value), "packed_pairs": int(vals[1].value), "strip_pairs": int(vals[2].value), "lane_use": vals[3].value,
                "trace_chunks": int(vals[4].value)}

    def set_chain(self, on: bool) -> None:
        """Chained strips for pairs with |b| > 1024 in run() and align_tiled() (align() ignores it).  Off by default."""
        self._check(self._fn("set_chain")(self._h, 1 if on else 0), f"{self._PREFIX}_set_chain")

    def chain_info(self) -> dict:
        """The setting, and the last chained pass: pairs and strip jobs run chained, chunks, boundary-row bytes of the largest chunk."""
        vals = [C.c_double(0) for _ in range(5)]
        self._fn("chain_info")(self._h, *[C.byref(v) for v in vals])
        d = {k: int(v.value) for k, v in zip(("on", "chain_pairs", "chain_jobs", "chunks", "bnd_bytes_max"), vals)}
        d["on"] = bool(d["on"])
        return d

    def set_free_ends(self, free_start: bool, free_end: bool) -> None:
        """Ends-free (semi-global) mode for every later run(), align() and align_tiled(): with free_start a prefix of a costs nothing
        (row 0 is zero), with free_end the cost is the lowest value of the last row and `end` the lowest column that holds it.  The
        CIGARs then describe a[start:end] against b (ends()).  Both off (the default): global alignment."""
        fs, fe = _switch(free_start, "free_start"), _switch(free_end, "free_end")
        self._check(self._fn("set_free_ends")(self._h, fs, fe), f"{self._PREFIX}_set_free_ends")

    def ends(self) -> np.ndarray:
        """int64[npairs, 2]: (start, end) of every pair in the last run(), align() or align_tiled() under the current setting; after a
        cost-only run() start is -1 under free_start and 0 otherwise.  ValueError before any such call or after set_free_ends."""
        n = max(self.npairs, 1)
        st, en = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self._check(self._fn("ends")(self._h, _p(st), _p(en)), f"{self._PREFIX}_ends")
        return np.stack([st, en], axis=1)[: self.npairs]

    def last_row(self, pairs=None) -> list:
        """M(i, |b|) for i = 0 .. |a| of every pair in `pairs` (indices; None: all), a list of int32 arrays, under the current setting: in
        global mode the cost of b against every prefix of a.  Runs a cost-only pass of its own, in chunks within
        PA_AFFINE_TRACE_BUDGET_MB; ValueError for a pair whose row alone exceeds it."""
        ids = list(range(self.npairs)) if pairs is None else [int(p) for p in pairs]
        if any(not 0 <= p < self.npairs for p in ids) or len(set(ids)) != len(ids):
            raise ValueError("pairs must be distinct indices of the batch")
        offs = np.full(max(self.npairs, 1), np.iinfo(np.uint64).max, np.uint64)
        total = 0
        for p in ids:
            offs[p] = total
            total += len(self._keep[p][0]) + 1
        out = np.zeros(max(total, 1), np.int32)
        self._check(self._fn("last_row")(self._h, _p(out), _p(offs)), f"{self._PREFIX}_last_row")
        return [out[int(offs[p]): int(offs[p]) + len(self._keep[p][0]) + 1].copy() for p in ids]

    @staticmethod
    def _s_max(s_max) -> int:
        return _s_max_arg(s_max)

    def run_dt(self, s_max: int) -> np.ndarray:
        """Costs only, by diagonal transition (WFA) bounded by s_max: int32[npairs], the cost of run() in global mode where it is
        <= s_max and -1 ("not found") where it is not.  No retry inside: the caller decides what to do with a -1.  The time is kept in
        `last_kernel_ms`, the counters in dt_info().  ValueError in ends-free mode."""
        s_max = self._s_max(s_max)
        costs = np.zeros(max(self.npairs, 1), np.int32)
        ms = C.c_float(0)
        self._check(self._fn("run_dt")(self._h, s_max, _p(costs), C.byref(ms)), f"{self._PREFIX}_run_dt")
        self.last_kernel_ms = float(ms.value)
        return costs[: self.npairs]

    def align_dt(self, s_max: int) -> list[tuple[int, str]]:
        """[(cost, CIGAR)] of every pair by diagonal transition bounded by s_max (trace batches only); (-1, "") where the cost exceeds
        s_max.  Same cost as align(); where several optimal paths exist the CIGAR may be another one of them (DEVIATIONS.md).  The
        times are kept in `last_forward_ms` and `last_trace_ms`."""
        s_max = self._s_max(s_max)
        L = load()
        n = self.npairs
        costs = np.zeros(max(n, 1), np.int32)
        cig = (C.c_void_p * max(n, 1))()
        f, t = C.c_float(0), C.c_float(0)
        rc = self._fn("align_dt")(self._h, s_max, _p(costs), cig, C.byref(f), C.byref(t))
        try:
            self._check(rc, f"{self._PREFIX}_align_dt")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        self.last_forward_ms, self.last_trace_ms = float(f.value), float(t.value)
        return [(int(costs[p]), cigars[p] if costs[p] >= 0 else "") for p in range(n)]

    def run_dt_ends(self, s_max: int, free_start: bool = True, free_end: bool = True) -> tuple[np.ndarray, np.ndarray]:
        """Costs and ends by ends-free diagonal transition bounded by s_max: (int32[npairs], int64[npairs]), the cost of run() and the
        end of ends() under set_free_ends(free_start, free_end) where the cost is <= s_max, and -1, -1 where it is not.  The switches
        belong to this call: the batch's own setting, ends() and every other route are left alone.  With both off: run_dt(), and
        end = |a|.  The time is kept in `last_kernel_ms`, the counters in dt_info()."""
        s_max = self._s_max(s_max)
        fs, fe = _switch(free_start, "free_start"), _switch(free_end, "free_end")
        costs, ends = np.zeros(max(self.npairs, 1), np.int32), np.zeros(max(self.npairs, 1), np.int64)
        ms = C.c_float(0)
        self._check(self._fn("run_dt_ends")(self._h, fs, fe, s_max, _p(costs), _p(ends), C.byref(ms)), f"{self._PREFIX}_run_dt_ends")
        self.last_kernel_ms = float(ms.value)
        return costs[: self.npairs], ends[: self.npairs]

    def align_dt_ends(self, s_max: int, free_start: bool = True, free_end: bool = True) -> list[tuple[int, str, int, int]]:
        """[(cost, CIGAR, start, end)] of every pair by ends-free diagonal transition bounded by s_max (trace batches only): b is placed
        in a[start:end], which the CIGAR describes; (-1, "", -1, -1) where the cost exceeds s_max.  Cost and end are those of align()
        under set_free_ends(free_start, free_end); start and the CIGAR may be another optimal placement (DEVIATIONS.md).  The times are
        kept in `last_forward_ms` and `last_trace_ms`."""
        s_max = self._s_max(s_max)
        fs, fe = _switch(free_start, "free_start"), _switch(free_end, "free_end")
        L = load()
        n = self.npairs
        costs = np.zeros(max(n, 1), np.int32)
        st, en = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        cig = (C.c_void_p * max(n, 1))()
        f, t = C.c_float(0), C.c_float(0)
        rc = self._fn("align_dt_ends")(self._h, fs, fe, s_max, _p(costs), _p(st), _p(en), cig, C.byref(f), C.byref(t))
        try:
            self._check(rc, f"{self._PREFIX}_align_dt_ends")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        self.last_forward_ms, self.last_trace_ms = float(f.value), float(t.value)
        return [(int(costs[p]), cigars[p] if costs[p] >= 0 else "", int(st[p]), int(en[p])) for p in range(n)]

    def dt_info(self) -> dict:
        """The last run_dt() / align_dt() or run_dt_ends() / align_dt_ends(): pairs found and not found, chunks, front cells computed (layers x live diagonals x cost
        steps), bytes compared while extending, device bytes of the largest chunk."""
        vals = [C.c_double(0) for _ in range(6)]
        self._fn("dt_info")(self._h, *[C.byref(v) for v in vals])
        return {k: int(v.value) for k, v in zip(("found", "not_found", "chunks", "front_cells", "extend_chars", "bytes_max"), vals)}

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AffineBatch(_AffineBatchBase):
    """Gap-affine global alignment of many pairs on the GPU (pa_affine_batch_*): NW::new(cm, false, false).align(a, b) of pa-base-algos
    for every pair, a and b in the orientation given (I consumes b, D consumes a).  trace=True allows align().  chain=True runs every
    pair with |b| > 1024 on a wavefront per strip of 1024 rows in run() and align_tiled() (set_chain); the results are the same.
    free_start / free_end (set_free_ends) make the ends of a, the text, free: the pattern b is placed in a[start:end]."""

    _PREFIX = "pa_affine_batch"
    _cost_c = staticmethod(AffineCost.to_c)

    def __init__(self, pairs, cm: AffineCost, trace: bool = False, chain: bool = False, free_start: bool = False, free_end: bool = False):
        free_start, free_end = _switch(free_start, "free_start"), _switch(free_end, "free_end")
        super().__init__(pairs, cm, trace)
        if chain:
            self.set_chain(True)
        if free_start or free_end:
            self.set_free_ends(free_start, free_end)

    def align_dt_seg(self, s_max: int, seg: int = 0, free_start: bool = False, free_end: bool = False) -> list[tuple[int, str, int, int]]:
        """align_dt_ends(s_max, free_start, free_end) in device memory that grows with the square root of the cost: the same
        [(cost, CIGAR, start, end)], byte for byte.  A checkpoint pass keeps the `largest edge` fronts below every segment of `seg`
        costs; then, segment by segment from the top, the fronts are computed again and walked.  seg = 0: about
        sqrt((bound + 1) * largest edge) per pair; else an integer in [largest edge, 2^30).  The times are kept in `last_forward_ms`
        (checkpoint pass), `last_refill_ms` (fills) and `last_trace_ms` (walks), the shape in dt_seg_info(), the checkpoint pass's
        counters in dt_info()."""
        s_max = self._s_max(s_max)
        if not isinstance(seg, (int, np.integer)) or isinstance(seg, (bool, np.bool_)) or not 0 <= seg < 1 << 30:
            raise ValueError(f"seg must be 0 or an integer in [largest edge, 2^30), got {seg!r}")
        fs, fe = _switch(free_start, "free_start"), _switch(free_end, "free_end")
        L = load()
        n = self.npairs
        costs = np.zeros(max(n, 1), np.int32)
        st, en = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        cig = (C.c_void_p * max(n, 1))()
        f, r, t = C.c_float(0), C.c_float(0), C.c_float(0)
        rc = L.pa_affine_batch_align_dt_seg(self._h, fs, fe, s_max, int(seg), _p(costs), _p(st), _p(en), cig, C.byref(f), C.byref(r), C.byref(t))
        try:
            self._check(rc, "pa_affine_batch_align_dt_seg")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        self.last_forward_ms, self.last_refill_ms, self.last_trace_ms = float(f.value), float(r.value), float(t.value)
        return [(int(costs[p]), cigars[p] if costs[p] >= 0 else "", int(st[p]), int(en[p])) for p in range(n)]

    def dt_seg_info(self) -> dict:
        """Shape of the last align_dt_seg(): chunks, rounds (a fill launch and a walk launch each), segment jobs, front cells the fills
        computed, device bytes of the largest chunk."""
        vals = [C.c_double(0) for _ in range(5)]
        load().pa_affine_batch_dt_seg_info(self._h, *[C.byref(v) for v in vals])
        return {k: int(v.value) for k, v in zip(("chunks", "rounds", "seg_jobs", "refill_cells", "bytes_max"), vals)}

    def run_local(self, match: int) -> tuple[np.ndarray, np.ndarray]:
        """Local (Smith-Waterman) alignment under the batch's cost model and a bonus of `match` per matching pair of bytes
        (include/pa_affine_local_hip.h), scores only: (scores int32[npairs], ends int64[npairs, 2] of (a_end, b_end)), the highest
        H(i, j) and its lowest i, then lowest j; score 0 is the empty alignment at (0, 0).  Independent of the batch's ends-free and
        chain settings.  The kernel time is kept in `last_kernel_ms`."""
        match = _match_arg(match)
        n = self.npairs
        scores = np.zeros(max(n, 1), np.int32)
        ae, be = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        ms = C.c_float(0)
        self._check(load().pa_affine_batch_run_local(self._h, match, _p(scores), _p(ae), _p(be), C.byref(ms)), "pa_affine_batch_run_local")
        self.last_kernel_ms = float(ms.value)
        return scores[:n], np.stack([ae[:n], be[:n]], axis=1)

    def align_local(self, match: int) -> list[tuple[int, str, int, int, int, int]]:
        """[(score, CIGAR, a_start, a_end, b_start, b_end)] of every pair's local alignment (trace batches only): the CIGAR describes
        a[a_start:a_end] against b[b_start:b_end], the clipped flanks are not printed.  In chunks whose traceback codes stay within
        PA_AFFINE_TRACE_BUDGET_MB (local_info()); ValueError naming a pair whose codes alone exceed it.  The times are kept in
        `last_forward_ms` and `last_trace_ms`."""
        match = _match_arg(match)
        L = load()
        n = self.npairs
        scores = np.zeros(max(n, 1), np.int32)
        ends = [np.zeros(max(n, 1), np.int64) for _ in range(4)]  # a_start, a_end, b_start, b_end
        cig = (C.c_void_p * max(n, 1))()
        f, t = C.c_float(0), C.c_float(0)
        rc = L.pa_affine_batch_align_local(self._h, match, _p(scores), *[_p(e) for e in ends], cig, C.byref(f), C.byref(t))
        try:
            self._check(rc, "pa_affine_batch_align_local")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        self.last_forward_ms, self.last_trace_ms = float(f.value), float(t.value)
        return [(int(scores[p]), cigars[p], *[int(e[p]) for e in ends]) for p in range(n)]

    def local_info(self) -> dict:
        """Shape of the last align_local(): chunks, device bytes of traceback codes of the largest one."""
        vals = [C.c_double(0) for _ in range(2)]
        load().pa_affine_batch_local_info(self._h, *[C.byref(v) for v in vals])
        return {k: int(v.value) for k, v in zip(("chunks", "bytes_max"), vals)}


def align_local(pairs, cm: AffineCost, match: int) -> list[tuple[int, str, int, int, int, int]]:
    """[(score, CIGAR, a_start, a_end, b_start, b_end)] of every pair's local alignment under the gap-affine cost model `cm` and a bonus
    of `match` per match: one traced AffineBatch (AffineBatch.align_local), or with a four-layer `cm` (AffineCost.double_affine) one
    traced Affine4Batch (Affine4Batch.align_sw)."""
    match = _match_arg(match)
    four = isinstance(cm, AffineCost) and len(cm.layers) == 4
    b = (Affine4Batch if four else AffineBatch)(pairs, cm, trace=True)
    try:
        return b.align_sw(match) if four else b.align_local(match)
    finally:
        b.close()


def align_affine(pairs, cm: AffineCost, tiled: bool = False, chain: bool = False, s_max: int | None = None) -> list[tuple[int, str]]:
    """[(cost, CIGAR)] of every pair under the gap-affine cost model `cm` (one traced AffineBatch); tiled=True takes the
    bounded-memory route (AffineBatch.align_tiled), for pairs whose whole code matrix would not fit.  chain=True (with tiled=True only:
    the untiled route has no chained form) chains the strips of the pairs with |b| > 1024 in the checkpoint pass.  s_max=K takes the
    diagonal-transition route instead (AffineBatch.align_dt(K), without tiled or chain): (-1, "") for a pair whose cost exceeds K."""
    if s_max is not None and (tiled or chain):
        raise ValueError("s_max selects the diagonal-transition route, which has no tiled or chained form")
    if chain and not tiled:
        raise ValueError("chain=True needs tiled=True: the untiled traced route has no chained form")
    b = AffineBatch(pairs, cm, trace=True, chain=chain)
    try:
        if s_max is not None:
            return b.align_dt(s_max)
        return b.align_tiled() if tiled else b.align()
    finally:
        b.close()


class Affine4Batch(_AffineBatchBase):
    """Double-affine (two-piece gap cost) global alignment of many pairs on the GPU (pa_affine4_batch_*): NW::new(cm, false,
    false).align(a, b) of pa-base-algos under an AffineCost<4> with layers [ins, del, ins, del] (AffineCost.double_affine, or four
    layers with costs of their own), a and b in the orientation given (I consumes b, D consumes a).  trace=True allows align() and
    align_tiled(), the same CIGARs in bounded device memory (include/pa_affine4_tiled_hip.h).  chain=True runs every pair with
    |b| > 1024 on a wavefront per strip of 1024 rows in run() and align_tiled() (set_chain, include/pa_affine4_chain_hip.h); the results
    are the same.  set_free_ends(free_start, free_end) (include/pa_affine4_ends_hip.h) makes the ends of a, the text, free in all of
    these routes: the pattern b is placed in a[start:end] (ends()), and last_row() gives M(i, |b|) of every column; map_affine does
    all of it in one call.  (The constructor keeps its four arguments, which tests/test_affine4_chain_api.py pins: the switches are set
    on the batch.)  run_dt(s_max) / align_dt(s_max) and run_dt_ends / align_dt_ends (include/pa_affine4_dt_hip.h) take the
    diagonal-transition route over the five layers, bounded by s_max: the choice for long pairs of low divergence (DESIGN.md has the
    measurements); map_affine_dt does the ends-free traced form in one call.  align_dt_segmented(s_max, seg) gives align_dt_ends' results
    in device memory that grows with the square root of the bound (include/pa_affine4_dt_seg_hip.h), for traced long pairs.
    run_sw(match) / align_sw(match) (include/pa_affine4_local_hip.h) are local (Smith-Waterman) alignment under the same costs and a
    bonus per match, AffineBatch.run_local / align_local's counterparts under names of their own; align_local(pairs, cm, match) picks
    the batch by the number of layers."""

    _PREFIX = "pa_affine4_batch"
    _WALK_MS = "last_walk_ms"
    _cost_c = staticmethod(AffineCost.to_c4)

    def __init__(self, pairs, cm: AffineCost, trace: bool = False, chain: bool = False):
        super().__init__(pairs, cm, trace)
        self.last_walk_ms = 0.0
        if chain:
            self.set_chain(True)

    def align_dt_segmented(self, s_max: int, seg: int = 0, free_start: bool = False, free_end: bool = False) -> list[tuple[int, str, int, int]]:
        """align_dt_ends(s_max, free_start, free_end) in device memory that grows with the square root of the bound: the same
        [(cost, CIGAR, start, end)], byte for byte (AffineBatch.align_dt_seg's counterpart).  A checkpoint pass keeps, below every
        segment of `seg` costs, the E fronts of the main layer and the extend_t fronts of layer t that the segment reads (E the largest
        of sub, ins, del and the opens; H rows in all); then, segment by segment from the top, the fronts are computed again and
        walked.  seg = 0: per pair the smallest S with 5 S^2 >= (bound + 1) H; else an integer in [Ew, 2^30), Ew the largest of E and
        the extends.  The times are kept in `last_forward_ms` (checkpoint pass), `last_refill_ms` (fills) and `last_trace_ms` (walks),
        the shape in dt_segmented_info(), the checkpoint pass's counters in dt_info()."""
        s_max = self._s_max(s_max)
        if not isinstance(seg, (int, np.integer)) or isinstance(seg, (bool, np.bool_)) or not 0 <= seg < 1 << 30:
            raise ValueError(f"seg must be 0 or an integer in [Ew, 2^30), got {seg!r}")
        fs, fe = _switch(free_start, "free_start"), _switch(free_end, "free_end")
        L = load()
        n = self.npairs
        costs = np.zeros(max(n, 1), np.int32)
        st, en = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        cig = (C.c_void_p * max(n, 1))()
        f, r, t = C.c_float(0), C.c_float(0), C.c_float(0)
        rc = L.pa_affine4_batch_align_dt_seg(self._h, fs, fe, s_max, int(seg), _p(costs), _p(st), _p(en), cig, C.byref(f), C.byref(r), C.byref(t))
        try:
            self._check(rc, "pa_affine4_batch_align_dt_seg")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        self.last_forward_ms, self.last_refill_ms, self.last_trace_ms = float(f.value), float(r.value), float(t.value)
        return [(int(costs[p]), cigars[p] if costs[p] >= 0 else "", int(st[p]), int(en[p])) for p in range(n)]

    def dt_segmented_info(self) -> dict:
        """Shape of the last align_dt_segmented(): chunks, rounds (a fill launch and a walk launch each), segment jobs, front cells the
        fills computed, device bytes of the largest chunk."""
        vals = [C.c_double(0) for _ in range(5)]
        load().pa_affine4_batch_dt_seg_info(self._h, *[C.byref(v) for v in vals])
        return {k: int(v.value) for k, v in zip(("chunks", "rounds", "seg_jobs", "refill_cells", "bytes_max"), vals)}

    def run_sw(self, match: int) -> tuple[np.ndarray, np.ndarray]:
        """Local (Smith-Waterman) alignment under the batch's two-piece gap costs and a bonus of `match` per matching pair of bytes
        (include/pa_affine4_local_hip.h; AffineBatch.run_local's counterpart), scores only: (scores int32[npairs], ends
        int64[npairs, 2] of (a_end, b_end)), the highest H(i, j) and its lowest i, then lowest j; score 0 is the empty alignment at
        (0, 0).  Independent of the batch's ends-free and chain settings.  The kernel time is kept in `last_kernel_ms`."""
        match = _match_arg(match)
        n = self.npairs
        scores = np.zeros(max(n, 1), np.int32)
        ae, be = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        ms = C.c_float(0)
        self._check(load().pa_affine4_batch_run_local(self._h, match, _p(scores), _p(ae), _p(be), C.byref(ms)), "pa_affine4_batch_run_local")
        self.last_kernel_ms = float(ms.value)
        return scores[:n], np.stack([ae[:n], be[:n]], axis=1)

    def align_sw(self, match: int) -> list[tuple[int, str, int, int, int, int]]:
        """[(score, CIGAR, a_start, a_end, b_start, b_end)] of every pair's local alignment (trace batches only; AffineBatch.align_local's
        counterpart): the CIGAR describes a[a_start:a_end] against b[b_start:b_end], gaps of different layers stay separate elements,
        the clipped flanks are not printed.  In chunks whose traceback codes stay within PA_AFFINE_TRACE_BUDGET_MB (sw_info());
        ValueError naming a pair whose codes alone exceed it.  The times are kept in `last_forward_ms` and `last_trace_ms`."""
        match = _match_arg(match)
        L = load()
        n = self.npairs
        scores = np.zeros(max(n, 1), np.int32)
        ends = [np.zeros(max(n, 1), np.int64) for _ in range(4)]  # a_start, a_end, b_start, b_end
        cig = (C.c_void_p * max(n, 1))()
        f, t = C.c_float(0), C.c_float(0)
        rc = L.pa_affine4_batch_align_local(self._h, match, _p(scores), *[_p(e) for e in ends], cig, C.byref(f), C.byref(t))
        try:
            self._check(rc, "pa_affine4_batch_align_local")
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
        self.last_forward_ms, self.last_trace_ms = float(f.value), float(t.value)
        return [(int(scores[p]), cigars[p], *[int(e[p]) for e in ends]) for p in range(n)]

    def sw_info(self) -> dict:
        """Shape of the last align_sw(): chunks, device bytes of traceback codes of the largest one."""
        vals = [C.c_double(0) for _ in range(2)]
        load().pa_affine4_batch_local_info(self._h, *[C.byref(v) for v in vals])
        return {k: int(v.value) for k, v in zip(("chunks", "bytes_max"), vals)}


def align_affine4(pairs, cm: AffineCost, trace: bool = True, tiled: bool = False):
    """Every pair under the four-layer cost model `cm` (one Affine4Batch): [(cost, CIGAR)] with trace=True, else the int32 costs.
    tiled=True takes align_tiled() (bounded device memory, the same CIGARs) and needs trace=True."""
    if tiled and not trace:
        raise ValueError("tiled=True needs trace=True: the tiled route is a traceback")
    b = Affine4Batch(pairs, cm, trace=trace)
    try:
        if not trace:
            return b.run()
        return b.align_tiled() if tiled else b.align()
    finally:
        b.close()


def map_affine(pairs, cm: AffineCost, free_start: bool = True, free_end: bool = True, tiled: bool = False, chain: bool = False,
               s_max: int | None = None) -> list[tuple[int, str, int, int]]:
    """[(cost, CIGAR, start, end)] of every pair (a the text, b the pattern) under the gap-affine cost model `cm` with the text's ends
    free (AffineBatch.set_free_ends): b is placed in a[start:end], which the CIGAR describes.  tiled and chain as in align_affine.
    A four-layer `cm` (AffineCost.double_affine) runs an Affine4Batch instead, tiled and chain likewise.
    s_max=K takes the diagonal-transition route instead (AffineBatch.align_dt_ends(K, free_start, free_end), without tiled or chain):
    (-1, "", -1, -1) for a pair whose cost exceeds K; ValueError with four layers, which have no such route."""
    free_start, free_end = _switch(free_start, "free_start"), _switch(free_end, "free_end")
    four = isinstance(cm, AffineCost) and len(cm.layers) == 4
    if four and s_max is not None:
        raise ValueError("s_max selects the diagonal-transition route, and diagonal transition has no double-affine route")
    if s_max is not None and (tiled or chain):
        raise ValueError("s_max selects the diagonal-transition route, which has no tiled or chained form")
    if chain and not tiled:
        raise ValueError("chain=True needs tiled=True: the untiled traced route has no chained form")
    if s_max is not None:
        s_max = _s_max_arg(s_max)
        b = AffineBatch(pairs, cm, trace=True)
        try:
            return b.align_dt_ends(s_max, free_start, free_end)
        finally:
            b.close()
    if four:
        b = Affine4Batch(pairs, cm, trace=True, chain=chain)
    else:
        b = AffineBatch(pairs, cm, trace=True, chain=chain, free_start=free_start, free_end=free_end)
    try:
        if four:
            b.set_free_ends(free_start, free_end)
        res = b.align_tiled() if tiled else b.align()
        se = b.ends()
        return [(c, g, int(se[p, 0]), int(se[p, 1])) for p, (c, g) in enumerate(res)]
    finally:
        b.close()


def map_affine_dt(pairs, cm: AffineCost, s_max: int, free_start: bool = True, free_end: bool = True) -> list[tuple[int, str, int, int]]:
    """[(cost, CIGAR, start, end)] of every pair (a the text, b the pattern) by ends-free diagonal transition bounded by s_max, under a
    model of at most two layers (one traced AffineBatch) or of four (one traced Affine4Batch): align_dt_ends(s_max, free_start,
    free_end) of either.  (-1, "", -1, -1) for a pair whose cost exceeds s_max."""
    s_max = _s_max_arg(s_max)
    free_start, free_end = _switch(free_start, "free_start"), _switch(free_end, "free_end")
    if not isinstance(cm, AffineCost):
        raise ValueError("cm must be an AffineCost")
    b = (Affine4Batch if len(cm.layers) == 4 else AffineBatch)(pairs, cm, trace=True)
    try:
        return b.align_dt_ends(s_max, free_start, free_end)
    finally:
        b.close()


def read_pairs(path: str) -> list[tuple[bytes, bytes]]:
    """Sequence pairs of a pa-bin input file or directory (.seq / .txt / .fna / .fa / .fasta; pa-bin/src/lib.rs:67-114)."""
    L = load()
    h = L.pa_pairs_read(str(path).encode())
    if not h:
        raise PaError(last_error())
    try:
        out = []
        for i in range(L.pa_pairs_count(h)):
            a, b, al, bl = C.c_void_p(None), C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
            L.pa_pairs_get(h, i, C.byref(a), C.byref(al), C.byref(b), C.byref(bl))
            out.append((C.string_at(a.value, al.value) if al.value else b"", C.string_at(b.value, bl.value) if bl.value else b""))
        return out
    finally:
        L.pa_pairs_free(h)


def align_file(input_path: str, output_path: str, params=None) -> int:
    """pa-bin's main loop on the GPU: every pair of the input gets one "{cost},{cigar}" line.  Returns the pair count.
    params: an AstarPa2Params (pa_align_file_params: batched A*PA2 for the `simple` family, a loop over pa_align otherwise)."""
    n = C.c_size_t(0)
    if params is not None:
        cp = params._to_c()
        rc = load().pa_align_file_params(str(input_path).encode(), str(output_path).encode(), C.byref(cp), C.byref(n))
    else:
        rc = load().pa_align_file(str(input_path).encode(), str(output_path).encode(), C.byref(n))
    if rc == -1:
        raise ValueError("sequence contains a character outside ACGT")
    if rc != 0:
        raise PaError(f"pa_align_file rc={rc}: {last_error()}")
    return int(n.value)


_str_from_c = C.pythonapi.PyUnicode_FromString  # C string -> str in one pass (string_at().decode() copies twice: 18 -> 9 ms per 10 000 CIGARs)
_str_from_c.restype = C.py_object
_str_from_c.argtypes = [C.c_void_p]


_str_from_c_n = C.pythonapi.PyUnicode_FromStringAndSize
_str_from_c_n.restype = C.py_object
_str_from_c_n.argtypes = [C.c_void_p, C.c_ssize_t]


def _c_strings(ptrs, n: int) -> list[str]:
    """The NUL-terminated strings a C call left in the pointer array `ptrs` (NULL -> "")."""
    return [_str_from_c(p) if p else "" for p in list(ptrs)[:n]]


class OperatorContext:
    """Device-resident operator handle (pa_bp_ctx_*): a, b, the profile and the stored h row stay on the GPU between calls."""

    H_NONE, H_INPUT, H_UPDATE, H_OUTPUT = 0, 1, 2, 3

    def __init__(self, a: bytes, b: bytes):
        L = load()
        self._keep = (a, b)
        self._h = L.pa_bp_ctx_create(C.cast(C.c_char_p(a), C.c_void_p), len(a), C.cast(C.c_char_p(b), C.c_void_p), len(b))
        if not self._h:
            raise PaError(last_error())

    @staticmethod
    def _check_v(v: np.ndarray, w0: int, w1: int) -> None:
        """The library reads and writes 16 * (w1 - w0) bytes at v: refuse anything that is not exactly that, in place."""
        if not isinstance(v, np.ndarray) or v.dtype != np.uint64 or v.shape != (w1 - w0, 2) or not v.flags["C_CONTIGUOUS"] or not v.flags["WRITEABLE"]:
            raise ValueError(f"v must be a writable C-contiguous uint64 array of shape ({w1 - w0}, 2)")

    def compute(self, i0: int, i1: int, w0: int, w1: int, v: np.ndarray, h_mode: int = 0) -> int:
        """v: uint64[w1 - w0, 2] (p, m), updated in place; returns the sum of the bottom-row deltas."""
        self._check_v(v, w0, w1)
        s = C.c_int32(0)
        rc = load().pa_bp_ctx_compute(self._h, i0, i1, w0, w1, _p(v), h_mode, C.byref(s))
        if rc != 0:
            raise PaError(f"pa_bp_ctx_compute rc={rc}: {last_error()}")
        return int(s.value)

    def fill(self, i0: int, i1: int, w0: int, w1: int, v: np.ndarray):
        """-> (values uint64[i1 - i0, w1 - w0, 2], bottom-row deltas int8[i1 - i0]); v updated in place."""
        self._check_v(v, w0, w1)
        values = np.zeros((i1 - i0, w1 - w0, 2), np.uint64)
        hb = np.zeros(max(i1 - i0, 1), np.int8)
        rc = load().pa_bp_ctx_fill(self._h, i0, i1, w0, w1, _p(v), _p(values), _p(hb))
        if rc != 0:
            raise PaError(f"pa_bp_ctx_fill rc={rc}: {last_error()}")
        return values, hb[: i1 - i0]

    def close(self):
        if self._h:
            load().pa_bp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def align_multi(pairs: list[tuple[bytes, bytes]], devices: list[int], trace: bool = True, params=None, stats: bool = False):
    """pa_batch_align_multi[_params]: a work queue of chunks of `pairs` served by one host thread per entry of `devices` (inside the
    library) -> (costs, CIGARs or None[, per-pair statistics]).  params: an AstarPa2Params of the `simple` family -> batched A*PA2."""
    L = load()
    n = len(pairs)
    if not devices or any(not isinstance(d, int) for d in devices):
        raise ValueError("devices must be a non-empty list of device indices")
    ap, al, bp, bl = _marshal_pairs(pairs)
    dev = (C.c_int * len(devices))(*devices)
    out = np.zeros(n, np.int32)
    cig = (C.c_void_p * n)() if trace else None
    st = None
    if params is not None:
        from .aligner import _StatsC

        cp = params._to_c()
        st = (_StatsC * max(n, 1))() if stats else None
        rc = L.pa_batch_align_multi_params(ap, al, bp, bl, n, dev, len(devices), C.byref(cp), _p(out), cig, st)
    else:
        rc = L.pa_batch_align_multi(ap, al, bp, bl, n, dev, len(devices), _p(out), cig)
    if rc == -1:
        raise ValueError("sequence contains a character outside ACGT")
    if rc != 0:
        raise PaError(f"pa_batch_align_multi rc={rc}: {last_error()}")
    cigars = None
    if trace:
        try:
            cigars = _c_strings(cig, n)
        finally:
            L.pa_free_cigars(cig, n)
    if st is not None:
        from .aligner import _StatsC

        return out, cigars, [{k: getattr(st[i], k) for k, _ in _StatsC._fields_} for i in range(n)]
    return out, cigars


class Batch:
    """Device-resident batch of independent pairs; run() = full-DP edit distance of every pair."""

    def __init__(self, pairs: list[tuple[bytes, bytes]], trace: bool = False, band: float | None = None, trace_params=None, params=None):
        """band: expected edit rate (e.g. 0.05) -> diagonal-band DP, re-run wider where it was too narrow (still exact).
        trace_params: an AstarPa2Params whose `front` (dt_trace, max_g, fr_drop) the batched traceback follows.
        params: an AstarPa2Params of the `simple` or `full` family -> batched A*PA2 (pa_batch_create_params): align() returns what a loop over
        AstarPa2(params).align(a, b) returns, pair_stats() the statistics."""
        L = load()
        self._keep = pairs
        self.trace = trace
        n = len(pairs)
        ap, al, bp, bl = _marshal_pairs(pairs)
        self.astar = params is not None
        if band is not None and trace:
            raise ValueError("banded batches are cost-only")
        if params is not None:
            cp = params._to_c()
            self.trace = True
            self._h = L.pa_batch_create_params(ap, al, bp, bl, n, C.byref(cp))
        elif band is not None:
            self._h = L.pa_batch_create_banded(ap, al, bp, bl, n, C.c_float(band))
        elif trace and trace_params is not None:
            cp = trace_params._to_c()
            self._h = L.pa_batch_create_trace_params(ap, al, bp, bl, n, C.byref(cp))
        else:
            self._h = (L.pa_batch_create_trace if trace else L.pa_batch_create)(ap, al, bp, bl, n)
        if not self._h:
            raise PaError(last_error())
        self.pairs = n

    def run(self):
        """-> (costs int32[pairs], strip-kernel milliseconds from HIP events)."""
        L = load()
        out = np.zeros(self.pairs, np.int32)
        ms = C.c_float(0)
        rc = L.pa_batch_run(self._h, _p(out), C.byref(ms))
        if rc == -1:
            raise ValueError("sequence contains a character outside ACGT")
        if rc != 0:
            raise PaError(f"pa_batch_run rc={rc}: {last_error()}")
        return out, float(ms.value)

    def align(self):
        """-> (costs int32[pairs], CIGAR strings, forward-kernel ms, traceback-kernel ms); needs trace=True.
        `self.last_c_abi_ms` = wall time of the C call itself (before Python turns the texts into str).  The call is pa_batch_align_view:
        the texts stay in the plan's host buffer and become str objects straight from there (pa_batch_align would malloc one C string per
        pair first, for Python to copy and free again)."""
        import time

        L = load()
        n = self.pairs
        out = np.zeros(n, np.int32)
        txt = (C.c_void_p * max(n, 1))()
        lens = np.zeros(max(n, 1), np.uint32)
        fms, tms = C.c_float(0), C.c_float(0)
        t0 = time.perf_counter()
        rc = L.pa_batch_align_view(self._h, _p(out), txt, _p(lens), C.byref(fms), C.byref(tms))
        self.last_c_abi_ms = (time.perf_counter() - t0) * 1e3
        if rc == -1:
            raise ValueError("sequence contains a character outside ACGT")
        if rc != 0:
            raise PaError(f"pa_batch_align_view rc={rc}: {last_error()}")
        cigars = [_str_from_c_n(p, l) if p else "" for p, l in zip(list(txt)[:n], lens[:n].tolist())]
        return out, cigars, float(fms.value), float(tms.value)

    def align_c_strings(self):
        """The same through pa_batch_align (one malloc'ed NUL-terminated string per pair, released with pa_free_cigars): the entry point a C
        caller of the reference's style uses.  -> (costs, CIGAR strings, forward-kernel ms, traceback-kernel ms)."""
        import time

        L = load()
        out = np.zeros(self.pairs, np.int32)
        cig = (C.c_void_p * max(self.pairs, 1))()
        fms, tms = C.c_float(0), C.c_float(0)
        t0 = time.perf_counter()
        rc = L.pa_batch_align(self._h, _p(out), cig, C.byref(fms), C.byref(tms))
        self.last_c_abi_ms = (time.perf_counter() - t0) * 1e3
        try:
            if rc == -1:
                raise ValueError("sequence contains a character outside ACGT")
            if rc != 0:
                raise PaError(f"pa_batch_align rc={rc}: {last_error()}")
            cigars = _c_strings(cig, self.pairs)
        finally:
            L.pa_free_cigars(cig, self.pairs)
        return out, cigars, float(fms.value), float(tms.value)

    def pair_stats(self) -> list[dict]:
        """AstarPa2Stats of every pair of the last align() (batches made with `params`)."""
        from .aligner import _StatsC

        arr = (_StatsC * max(self.pairs, 1))()
        rc = load().pa_batch_pair_stats(self._h, arr)
        if rc != 0:
            raise PaError(f"pa_batch_pair_stats rc={rc}: {last_error()}")
        return [{n: getattr(arr[i], n) for n, _ in _StatsC._fields_} for i in range(self.pairs)]

    def full_info(self) -> dict:
        """pa_batch_full_info: reporting for batches of the `full` family."""
        vals = [C.c_double(0) for _ in range(4)]
        ph = (C.c_double * 8)()
        load().pa_batch_full_info(self._h, *[C.byref(v) for v in vals], ph)
        d = dict(zip(("build_ms", "matches", "probes", "rounds"), (v.value for v in vals)))
        d["phase_wave_ms"] = dict(zip(("contours", "dp", "h", "index", "prune", "init", "total"), [x for x in ph][:7]))
        return d

    def rdv_stats(self) -> dict:
        """pa_batch_rdv_stats: how the half-wave blocks of the last forward pass met (batched A*PA2; diagnostics)."""
        out = (C.c_uint64 * 4)()
        rc = load().pa_batch_rdv_stats(self._h, out)
        if rc != 0:
            raise PaError(f"pa_batch_rdv_stats rc={rc}: {last_error()}")
        return dict(zip(("fused", "served", "alone", "withdrawn"), (int(x) for x in out)))

    def trace_fallbacks(self) -> int:
        return int(load().pa_batch_trace_fallbacks(self._h))

    def window_retry_bytes(self) -> float:
        """The largest full-height block-column store a second round (pairs whose band left their window) of this plan held at a time."""
        f = load().pa_batch_window_retry_bytes
        f.argtypes, f.restype = [C.c_void_p], C.c_double
        return float(f(self._h))

    def window_retries(self) -> int:
        """Pairs whose band left their window of the block-column store and were aligned again with full-height columns."""
        return int(load().pa_batch_window_retries(self._h))

    def stats(self) -> dict:
        vals = [C.c_double(0) for _ in range(4)]
        load().pa_batch_stats(self._h, *[C.byref(v) for v in vals])
        return dict(zip(("cells", "word_updates", "strips", "algo_bytes"), (v.value for v in vals)))

    def shape(self) -> dict:
        """How the batch was laid out: strip height k, chained strips or one wavefront per pair, VALU instructions per pass."""
        k, seq, vi = C.c_int(0), C.c_int(0), C.c_double(0)
        load().pa_batch_shape(self._h, C.byref(k), C.byref(seq), C.byref(vi))
        sl = [C.c_double(0) for _ in range(5)]
        rows = load().pa_batch_slice_info(self._h, *[C.byref(v) for v in sl])
        if rows:  # groups of 32 pairs, bit-sliced (csrc/slice_kernel.hpp)
            return {"k": 0, "sequential": False, "valu_instructions": vi.value, "kernel": f"pa::slice::slice_kernel<{rows}>", "sliced_rows_per_lane": rows,
                    "groups": int(sl[0].value), "jobs": int(sl[1].value), "computed_cells": sl[2].value, "device_bytes": sl[3].value,
                    "boundary_bytes": sl[4].value}
        return {"k": k.value, "sequential": bool(seq.value), "valu_instructions": vi.value,
                "kernel": f"pa::pair_kernel<{k.value}>" if seq.value else f"pa::strip_kernel<{k.value}, false, false>"}

    def close(self):
        if self._h:
            load().pa_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
