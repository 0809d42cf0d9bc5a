"""Batched semi-global search (pa.SearchBatch) on the four shapes of its issue, against a Python loop over pa.search and against the
same batch with packing switched off (PA_SEARCH_BATCH_NO_PACK=1: every query on strips of its own).

    python tools/search_batch_bench.py [--shapes reads,kbp,10kbp,primers] [--repeats 5] [--loop-queries 200]

Prints one JSON line per (shape, mode): queries/s from the median of `repeats` timed runs after one warm-up run (the kernel time of
pa_search_batch_run's HIP events and the wall time of run()), cells/s = sum plen * tlen over the kernel time, and the plan's lane use.
For kernel-only figures run it under `rocprofv3 --kernel-trace --stats` on its own.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

import astar_pairwise_aligner_amd as pa  # noqa: E402
from astar_pairwise_aligner_amd.generate import mutate, random_sequence  # noqa: E402


def shape(name: str):
    """-> (patterns, texts, queries)"""
    rng = np.random.default_rng(1)
    if name in ("reads", "kbp", "10kbp"):
        n, plen, win = {"reads": (100_000, 150, 500), "kbp": (10_000, 1000, 5000), "10kbp": (1_000, 10_000, 30_000)}[name]
        genome = random_sequence(max(n * 37, 4 * win), seed=7)
        pats, texts = [], []
        for k in range(n):
            at = int(rng.integers(0, len(genome) - win))
            w = genome[at: at + win]
            off = (win - plen) // 2
            pats.append(mutate(w[off: off + plen], 0.05, k))
            texts.append(w)
        return pats, texts, [(k, k) for k in range(n)]
    if name == "primers":
        genome = random_sequence(5_000_000, seed=9)
        pats = []
        for k in range(100):
            at = int(rng.integers(0, len(genome) - 25))
            pats.append(mutate(genome[at: at + 25], 0.04, k))
        return pats, [genome], [(k, 0) for k in range(100)]
    raise ValueError(name)


def measure(pats, texts, queries, repeats: int, no_pack: bool) -> dict:
    if no_pack:
        os.environ["PA_SEARCH_BATCH_NO_PACK"] = "1"
    else:
        os.environ.pop("PA_SEARCH_BATCH_NO_PACK", None)
    t0 = time.perf_counter()
    sb = pa.SearchBatch(pats, texts, queries, 0.0)
    create_s = time.perf_counter() - t0
    sb.run()  # warm-up
    kms, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        sb.run()
        wall.append(time.perf_counter() - t0)
        kms.append(sb.last_kernel_ms)
    info = sb.info()
    sb.close()
    os.environ.pop("PA_SEARCH_BATCH_NO_PACK", None)
    cells = float(sum(len(pats[i]) * len(texts[j]) for i, j in queries))
    k_s = statistics.median(kms) / 1e3
    return {"mode": "no_pack" if no_pack else "packed", "queries": len(queries), "create_s": round(create_s, 3),
            "kernel_ms_median": round(k_s * 1e3, 3), "kernel_ms_min": round(min(kms), 3), "run_wall_ms_median": round(statistics.median(wall) * 1e3, 3),
            "queries_per_s": round(len(queries) / statistics.median(wall), 1), "cells_per_s_kernel": cells / k_s if k_s > 0 else None,
            **info}


def loop(pats, texts, queries, n: int) -> dict:
    sel = queries[:: max(1, len(queries) // n)][:n]
    pa.search(pats[sel[0][0]], texts[sel[0][1]], 0.0)  # warm-up
    t0 = time.perf_counter()
    for i, j in sel:
        pa.search(pats[i], texts[j], 0.0)
    dt = time.perf_counter() - t0
    return {"mode": "python_loop_pa_search", "queries_timed": len(sel), "queries_per_s": round(len(sel) / dt, 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reads,kbp,10kbp,primers")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-queries", type=int, default=200)
    ap.add_argument("--no-compare", action="store_true", help="packed batch only")
    a = ap.parse_args()
    pa.require_gpu()
    for name in a.shapes.split(","):
        pats, texts, queries = shape(name)
        rows = [measure(pats, texts, queries, a.repeats, False)]
        if not a.no_compare:
            rows.append(measure(pats, texts, queries, a.repeats, True))
            rows.append(loop(pats, texts, queries, a.loop_queries))
        for r in rows:
            print(json.dumps({"shape": name, **r}), flush=True)


if __name__ == "__main__":
    main()
