"""Batched gap-affine alignment (pa_affine_batch_*): kernel time, GCUPS and pairs/s, costs only and traced, for three shapes under
affine(4, 6, 2) and unit(), next to one CPU core running a plain scalar Gotoh (C, built here with the system compiler).

    python tools/affine_bench.py [--shapes reads,10k,100k,100k1] [--trace-100k] [--tile-cols C] [--reps R] [--chain] [--ends] [--dt] [--dt-ends]
                                 [--dt-seg] [--double] [--double-tiled] [--double-chain] [--double-ends] [--double-dt] [--double-dt-ends] [--double-dt-seg]
                                 [--local] [--double-local]
                                 [--models affine,unit]

Cells are |a| |b| per pair.  Traced times are the forward (code-writing) kernels plus the walks, summed over the budget's chunks; the
tiled route's are its checkpoint pass, tile fills and walks.  Both routes run on one batch, each warmed once and then R times in turn;
the line shows the fastest repeat and lists them all.  The tiled route also traces what the untiled one leaves out: all pairs of the
10 kbp shape and the 100 kbp shape (once, unwarmed: a pass over those takes seconds).

--chain measures the chained route (AffineBatch.set_chain) instead: for each shape the cost-only pass and the tiled traced pass with
chaining off and on, on one batch in one process, alternating, each warmed once and then R times; it prints both routes' fastest
repeats, their ratio and chain_info().  The shape 100k1 is one 100 kbp pair.

--ends measures the ends-free mode (AffineBatch.set_free_ends, both ends of the text free) on two mapping shapes of its own, whatever
--shapes says: 100 000 patterns of 150 bp in 400 bp windows, and 4096 reads of 10 kbp in 12 kbp windows (traced: --trace-pairs of them).
Each runs cost-only, traced and tiled, global and ends-free alternating on one batch, each warmed once and then R times: the cells are
the same, so the ratio of the fastest repeats is what the mode costs.

--dt measures the diagonal-transition route (AffineBatch.run_dt) against run() instead: for each shape one batch in one process, run() and
run_dt() alternating, each warmed once and then three times; s_max is the largest cost run() returned for the batch, so every pair is
found.  run() is chained for the 100 kbp shapes (its best route there).  It prints both routes' fastest repeats, their ratio (above 1:
DT is faster) and dt_info().  A shape takes a divergence in per cent after an @: 10k@1, 10k@15, reads@15 (default 5).

--dt-ends measures the ends-free diagonal-transition route (AffineBatch.run_dt_ends) against the ends-free run() on the mapping shapes of
--ends: map150 (100 000 x 150 bp in 400 bp windows) and map10k@1, map10k@3, map10k@5 (4096 x 10 kbp in 12 kbp windows), or those of
them that --shapes names.  Each runs twice: both ends free on the windows, and free_end only on the windows cut to begin where the
pattern does (extension from a seed: front 0 is one diagonal).  One batch, run() and run_dt_ends(largest cost) alternating, each
warmed once and then three times; the costs and ends of the two routes must agree.

--dt-seg measures the segmented traceback of the diagonal-transition route (AffineBatch.align_dt_seg, default seg) against
AffineBatch.align_dt_ends, globally, on the shapes of --shapes (a divergence after an @ as for --dt): one traced batch in one process,
s_max the largest cost run_dt() finds, the two calls in turn, each warmed once and then three times, the results compared in every round.
It prints both calls' fastest repeat with its parts, the ratio of the totals next to the ratio of the two bytes_max, rounds and chunks.
Where align_dt_ends refuses the batch (a pair's fronts exceed the budget) its error is printed and align_dt_seg runs alone.

--double measures the double-affine batch (Affine4Batch under double_affine(4, 6, 2, 24, 1)) against AffineBatch under affine(4, 6, 2),
whatever --shapes says: 100 000 x 150 bp and 4096 x 10 kbp at 5 %, a quarter of the pairs with one more indel of 20 to 200 bytes so that
layers 2 and 3 are used.  Both batches hold the same pairs; run() alternates between them, each warmed once and then three times, and
the line shows the fastest repeats, their ratio (double over affine) and how many pairs differ in cost between the two models.  align()
does the same on --trace-pairs of the 10 kbp pairs.

--double-tiled measures the tiled traceback of the double-affine batch (Affine4Batch.align_tiled) on the 10 kbp pairs of --double:
align() and align_tiled() alternating on one batch of --trace-pairs of them, each warmed once and then three times, the fastest repeat
of each, their ratio, and the results compared in every round; then align_tiled() alone on all 4096 pairs, and on 16 pairs of 100 kbp
(once, unwarmed, in a process of its own under a time limit of two lone-wavefront passes).  Every leg prints tiled_info(): chunks,
rounds, tile jobs, the cells re-filled and the bytes of the largest chunk, also per pair.

--double-chain is --chain's protocol on an Affine4Batch under double_affine(4, 6, 2, 24, 1) (Affine4Batch.set_chain), whatever --shapes
says: one 100 kbp pair, 16 of them, 4096 x 10 kbp and the reads (which have no pair to chain), with the long indels of --double.  Cost
only, the tiled forward pass and traced in all, chained and unchained alternating on one batch, each warmed once and then R times, the
results compared in every round.  Every shape runs in a process of its own under a wall-clock limit sized for its unchained passes (a
100 kbp pair alone on a wavefront takes 7 to 10 s a pass).

--local measures what local alignment costs over the global mode (AffineBatch.run_local / align_local at match = 2), whatever --shapes
says: 100 000 x 150 bp reads in 400 bp windows (cost-only and traced), 4096 x 10 kbp cost-only and --trace-pairs of them traced.  On one
batch, run() against run_local() and align() against align_local(), alternating, each warmed once and then three times; the fastest
repeat of each and their ratio.

--double-local is --local's protocol and shapes on an Affine4Batch under double_affine(4, 6, 2, 24, 1): run() against run_sw(2) and align()
against align_sw(2), alternating on one batch.

--double-ends is --ends' protocol and mapping shapes on an Affine4Batch under double_affine(4, 6, 2, 24, 1) (Affine4Batch.set_free_ends):
cost-only, traced and tiled (at --tile-cols, by default the library's 1024), global and ends-free alternating on one batch.

--double-dt is --dt's protocol on an Affine4Batch under double_affine(4, 6, 2, 24, 1) (Affine4Batch.run_dt), whatever --shapes says (or the
shapes of --shapes that carry an @): reads@5, 10k@1, 10k@3, 10k@5, 10k@8 and 100k@5 with run() chained.  One batch in one process, run() and
run_dt(largest cost) alternating, each warmed once and then three times; the fastest repeats, their ratio and dt_info().  The same pairs
then go through AffineBatch.run_dt under affine(4, 6, 2) at that model's largest cost, the second column: what five layers cost over three.

--double-dt-ends does likewise against the ends-free run() (Affine4Batch.run_dt_ends, both ends free) on the mapping shapes of --dt-ends:
map150, map10k@1, map10k@3, map10k@5.

--double-dt-seg is --dt-seg's protocol on an Affine4Batch under double_affine(4, 6, 2, 24, 1) (Affine4Batch.align_dt_segmented, default seg,
against Affine4Batch.align_dt_ends), whatever --shapes says (or the shapes of --shapes that carry an @): 10k@1, 10k@3, 10k@5, reads@5
and 100k@5.  Where align_dt_ends refuses the batch its error is printed and align_dt_segmented runs alone."""
from __future__ import annotations

import argparse
import ctypes as C
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import astar_pairwise_aligner_amd as pa  # noqa: E402
from astar_pairwise_aligner_amd import Affine4Batch, AffineBatch, AffineCost  # noqa: E402

GOTOH_C = r"""
#include <stdint.h>
#include <stdlib.h>
/* cost of the global alignment, column by column over a; absent edge = 1 << 30 (INF) */
int64_t gotoh(const uint8_t* a, int64_t n, const uint8_t* b, int64_t m, int64_t sub, int64_t ins, int64_t del, int64_t io, int64_t ie,
              int64_t dop, int64_t de) {
    const int64_t INF = 1 << 30;
    int64_t *M = malloc((m + 1) * sizeof(int64_t)), *D = malloc((m + 1) * sizeof(int64_t));
    M[0] = 0; D[0] = INF;
    int64_t I = INF;
    for (int64_t j = 1; j <= m; ++j) {
        I = I + ie < M[j - 1] + io ? I + ie : M[j - 1] + io;
        int64_t v = M[j - 1] + ins; if (I + ie < v) v = I + ie; M[j] = v < INF ? v : INF; D[j] = INF;
    }
    for (int64_t i = 1; i <= n; ++i) {
        int64_t diag = M[0];
        D[0] = D[0] + de < M[0] + dop ? D[0] + de : M[0] + dop;
        int64_t v0 = M[0] + del; if (D[0] + de < v0) v0 = D[0] + de; M[0] = v0 < INF ? v0 : INF;
        I = INF;
        const uint8_t ai = a[i - 1];
        for (int64_t j = 1; j <= m; ++j) {
            I = I + ie < M[j - 1] + io ? I + ie : M[j - 1] + io;
            D[j] = D[j] + de < M[j] + dop ? D[j] + de : M[j] + dop;
            int64_t v = diag + (ai == b[j - 1] ? 0 : sub);
            if (M[j - 1] + ins < v) v = M[j - 1] + ins;
            if (M[j] + del < v) v = M[j] + del;
            if (I + ie < v) v = I + ie;
            if (D[j] + de < v) v = D[j] + de;
            diag = M[j];
            M[j] = v < INF ? v : INF;
        }
    }
    int64_t r = M[m];
    free(M); free(D);
    return r;
}
"""


def cpu_lib():
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        return None
    d = Path(tempfile.mkdtemp())
    (d / "gotoh.c").write_text(GOTOH_C)
    subprocess.run([cc, "-O3", "-march=native", "-shared", "-fPIC", "-o", str(d / "gotoh.so"), str(d / "gotoh.c")], check=True)
    L = C.CDLL(str(d / "gotoh.so"))
    L.gotoh.restype = C.c_int64
    L.gotoh.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64] + [C.c_int64] * 7
    return L


def cpu_args(cm):
    il, dl = cm.ins_layer(), cm.del_layer()
    inf = 1 << 30
    z = lambda v: inf if v is None else v  # noqa: E731
    return [z(cm.sub), z(cm.ins), z(cm.del_), z(il and il[0]), z(il and il[1]), z(dl and dl[0]), z(dl and dl[1])]


def rand_seq(rng, n):
    return bytes(b"ACGT"[k] for k in rng.integers(0, 4, n)) if n < 5000 else np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def mutate(rng, s: bytes, rate: float) -> bytes:
    x = np.frombuffer(s, np.uint8)
    r = rng.random(len(x))
    keep = r >= rate / 3  # deletions
    out = x.copy()
    subm = (r >= rate / 3) & (r < 2 * rate / 3)
    out[subm] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(subm.sum()))]
    ins = (r >= 2 * rate / 3) & (r < rate)
    pieces = np.where(ins[:, None], np.stack([out, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(x))]], 1), out[:, None])
    flat = [pieces[k, : 2 if ins[k] else 1] for k in range(len(x)) if keep[k]] if len(x) < 5000 else None
    if flat is not None:
        return b"".join(p.tobytes() for p in flat)
    lens = np.where(keep, np.where(ins, 2, 1), 0)
    idx = np.repeat(np.arange(len(x)), lens)
    second = np.concatenate([[False], idx[1:] == idx[:-1]])
    return np.where(second, pieces[idx, 1], pieces[idx, 0]).astype(np.uint8).tobytes()


def shape(name, rng):
    name, _, pct = name.partition("@")
    rate = float(pct) / 100 if pct else 0.05
    pct = pct or "5"
    if name == "reads":
        pairs = []
        for _ in range(100_000):
            w = int(rng.integers(150, 201))
            y = rand_seq(rng, w)
            pairs.append((mutate(rng, y[:150], rate), y))
        return "100000 x 150 bp reads vs 150-200 bp windows" + ("" if pct == "5" else f" at {pct} %"), pairs
    if name == "10k":
        pairs = []
        for _ in range(4096):
            y = rand_seq(rng, 10_000)
            pairs.append((mutate(rng, y, rate), y))
        return f"4096 x 10 kbp at {pct} %", pairs
    pairs = []
    for _ in range(1 if name == "100k1" else 16):
        y = rand_seq(rng, 100_000)
        pairs.append((mutate(rng, y, rate), y))
    return f"{len(pairs)} x 100 kbp at {pct} %", pairs


def long_indels(rng, pairs, share=0.25):
    """An indel of 20 to 200 bytes in a share of the pairs: bytes put into a, or taken out of it, at a random place."""
    out = []
    for x, y in pairs:
        if rng.random() < share:
            L = int(rng.integers(20, 201))
            if rng.random() < 0.5 or len(x) < L + 20:
                at = int(rng.integers(0, len(x) + 1))
                x = x[:at] + rand_seq(rng, L) + x[at:]
            else:
                at = int(rng.integers(0, len(x) - L + 1))
                x = x[:at] + x[at + L:]
        out.append((x, y))
    return out


def double_legs(title, pairs, tp):
    """Affine4Batch under double_affine(4, 6, 2, 24, 1) against AffineBatch under affine(4, 6, 2) on the same pairs, alternating, each
    warmed once and then three times: run() on all pairs, align() on the pairs tp."""
    cm2, cm4 = AffineCost.affine(4, 6, 2), AffineCost.double_affine(4, 6, 2, 24, 1)
    cells = float(sum(len(x) * len(y) for x, y in pairs))
    b2, b4 = AffineBatch(pairs, cm2), Affine4Batch(pairs, cm4)
    t2, t4 = [], []
    for rep in range(4):  # the first round warms both
        c2 = b2.run()
        k2 = b2.last_kernel_ms
        c4 = b4.run()
        if rep:
            t2.append(k2)
            t4.append(b4.last_kernel_ms)
    info = b4.info()
    b2.close()
    b4.close()
    if (c4 > c2).any():
        raise SystemExit(f"{title}: a double-affine cost above the two-layer cost")
    k2, k4 = min(t2), min(t4)
    print(f"{title:52s} run():   affine(4,6,2) {k2:10.2f} ms {cells / k2 / 1e6:8.1f} GCUPS | double_affine(4,6,2,24,1) {k4:10.2f} ms"
          f" {cells / k4 / 1e6:8.1f} GCUPS | ratio {k4 / k2:6.3f}  (repeats {' '.join(f'{x:.2f}' for x in t2)} | {' '.join(f'{x:.2f}' for x in t4)})", flush=True)
    print(f"{'':52s} {int((c4 != c2).sum())} of {len(pairs)} pairs differ in cost between the two models (mean cost {float(c2.mean()):.1f} and"
          f" {float(c4.mean()):.1f}); plan {info}", flush=True)
    if tp is None:
        return
    cells = float(sum(len(x) * len(y) for x, y in tp))
    b2, b4 = AffineBatch(tp, cm2, trace=True), Affine4Batch(tp, cm4, trace=True)
    t2, t4 = [], []
    for rep in range(4):
        r2 = b2.align()
        f2 = (b2.last_forward_ms, b2.last_trace_ms)
        r4 = b4.align()
        if rep:
            t2.append(f2)
            t4.append((b4.last_forward_ms, b4.last_trace_ms))
    chunks = (b2.info()["trace_chunks"], b4.info()["trace_chunks"])
    b2.close()
    b4.close()
    (f2, w2), (f4, w4) = min(t2, key=sum), min(t4, key=sum)
    differ = sum(x[0] != y[0] for x, y in zip(r2, r4))
    print(f"{'':52s} align() of {len(tp)} pairs: affine forward {f2:9.2f} ms + walks {w2:7.2f} ms | double_affine forward {f4:9.2f} ms + walks"
          f" {w4:7.2f} ms | ratio forward {f4 / f2:6.3f}, all {(f4 + w4) / (f2 + w2):6.3f}  ({cells / (f4 + w4) / 1e6:.1f} GCUPS traced; chunks {chunks};"
          f" {differ} pairs differ in cost; repeats {' '.join(f'{sum(x):.2f}' for x in t2)} | {' '.join(f'{sum(x):.2f}' for x in t4)})", flush=True)


def double_tiled_leg(title, tp, untiled, tile_cols, warm=True, reps=3):
    """Affine4Batch.align() (if `untiled`) and align_tiled() under double_affine(4, 6, 2, 24, 1), alternating on one batch, each warmed once
    (if `warm`) and then `reps` times; the fastest repeat of each, their ratio, and tiled_info().  -> the tiled route's fastest time."""
    cm4 = AffineCost.double_affine(4, 6, 2, 24, 1)
    cells = float(sum(len(x) * len(y) for x, y in tp))
    b = Affine4Batch(tp, cm4, trace=True)
    un, ti = [], []
    base = None
    for rep in range(reps + (1 if warm else 0)):
        if untiled:
            base = b.align()
            u = (b.last_forward_ms, b.last_trace_ms)
        got = b.align_tiled(tile_cols)
        if untiled and got != base:
            raise SystemExit(f"{title}: align_tiled() differs from align()")
        if rep or not warm:
            if untiled:
                un.append(u)
            ti.append((b.last_forward_ms, b.last_refill_ms, b.last_walk_ms))
    info, chunks = b.tiled_info(), b.info()["trace_chunks"]
    b.run()
    run_ms = b.last_kernel_ms
    b.close()
    f, r, w = min(ti, key=sum)
    t = f + r + w
    line = f"{title:52s} align_tiled() of {len(tp)} pairs: {t:10.2f} ms = checkpoint pass {f:.2f} + fills {r:.2f} + walks {w:.2f}  ({cells / t / 1e6:.1f} GCUPS"
    line += f"; run() {run_ms:.2f} ms, checkpoint pass over run() {f / run_ms:.3f}"
    if untiled:
        uf, uw = min(un, key=sum)
        line += f") | align() {uf + uw:10.2f} ms = forward {uf:.2f} + walks {uw:.2f}, {chunks} chunks | ratio tiled over untiled {t / (uf + uw):6.3f}  ("
        line += f"repeats {' '.join(f'{sum(x):.2f}' for x in un)} | {' '.join(f'{sum(x):.2f}' for x in ti)}"
    else:
        line += f"; repeats {' '.join(f'{sum(x):.2f}' for x in ti)}" + ("" if warm else ", unwarmed")
    print(line + ")", flush=True)
    print(f"{'':52s} tiled: {info['chunks']} chunks, {info['rounds']} rounds, {info['tile_jobs']} tile jobs, {info['refill_cells'] / 1e9:.2f} G cells"
          f" re-filled ({info['refill_cells'] / cells:.3f} of the matrix), largest chunk {info['chunk_bytes_max']} bytes"
          f" ({info['chunk_bytes_max'] / len(tp) / 1e6:.3f} MB per pair)", flush=True)
    return t


# The 100 kbp leg of --double-tiled: a pair's checkpoint pass runs on one wavefront (chaining is off by default; --double-chain measures it on), about 7 s
# for the two-layer kernel times the four-layer ratio of 1.3; the limit is two such passes.
DOUBLE_100K_LIMIT_S = 2 * 7.0 * 1.3


def chain_legs(title, pairs, cm, mname, tile_cols, reps, Batch=AffineBatch):
    """Chaining off and on, alternating on one traced batch: run() and align_tiled()."""
    cells = float(sum(len(x) * len(y) for x, y in pairs))
    b = Batch(pairs, cm, trace=True)
    cost = {False: [], True: []}
    tiled = {False: [], True: []}
    results = {}
    for rep in range(reps + 1):  # the first round warms both routes
        for on in (False, True):
            b.set_chain(on)
            c = b.run()
            k = b.last_kernel_ms
            t = b.align_tiled(tile_cols)
            results.setdefault("cost", c.tolist())
            results.setdefault("tiled", t)
            if c.tolist() != results["cost"] or t != results["tiled"]:
                raise SystemExit(f"{title} {mname}: the chained and the unchained route disagree")
            if rep:
                cost[on].append(k)
                tiled[on].append((b.last_forward_ms, b.last_refill_ms, getattr(b, b._WALK_MS)))
    ci = b.chain_info()
    b.close()
    k0, k1 = min(cost[False]), min(cost[True])
    print(f"{title:44s} {mname:14s} cost-only: unchained {k0:10.2f} ms {cells / k0 / 1e6:8.1f} GCUPS | chained {k1:10.2f} ms {cells / k1 / 1e6:8.1f} GCUPS"
          f" | ratio {k0 / k1:7.2f}  (repeats {' '.join(f'{x:.2f}' for x in cost[False])} | {' '.join(f'{x:.2f}' for x in cost[True])})", flush=True)
    (f0, r0, w0), (f1, r1, w1) = min(tiled[False], key=sum), min(tiled[True], key=sum)
    print(f"{'':44s} {mname:14s} tiled:     unchained forward {f0:10.2f} ms, all {f0 + r0 + w0:10.2f} ms | chained forward {f1:10.2f} ms, all"
          f" {f1 + r1 + w1:10.2f} ms | ratio forward {f0 / f1:7.2f}, all {(f0 + r0 + w0) / (f1 + r1 + w1):7.2f}"
          f"  (fills {r1:.2f} ms, walks {w1:.2f} ms; repeats {' '.join(f'{sum(x):.2f}' for x in tiled[False])} |"
          f" {' '.join(f'{sum(x):.2f}' for x in tiled[True])})", flush=True)
    print(f"{'':44s} {mname:14s} chain_info: {ci}", flush=True)


# --double-chain: a shape's process may take its pairs (a minute of Python at most) and, per round, four passes (run() and align_tiled(),
# unchained and chained) of which the two unchained ones are lone-wavefront passes.
DOUBLE_CHAIN_SHAPES = ("100k1", "100k", "10k", "reads")


def double_chain_limit_s(reps):
    return 60 + (reps + 1) * 2 * DOUBLE_100K_LIMIT_S


def dt_legs(title, pairs, cm, mname, chain):
    """run() and run_dt(largest cost), alternating on one batch."""
    cells = float(sum(len(x) * len(y) for x, y in pairs))
    b = AffineBatch(pairs, cm, chain=chain)
    want = b.run()
    s_max = int(want.max())
    nw, dt = [], []
    for rep in range(4):  # the first round warms both routes
        c = b.run()
        k = b.last_kernel_ms
        d = b.run_dt(s_max)
        if c.tolist() != want.tolist() or d.tolist() != want.tolist():
            raise SystemExit(f"{title} {mname}: run() and run_dt() disagree")
        if rep:
            nw.append(k)
            dt.append(b.last_kernel_ms)
    di = b.dt_info()
    b.close()
    k0, k1 = min(nw), min(dt)
    print(f"{title:44s} {mname:14s} run(){' chained' if chain else ''}: {k0:10.2f} ms {cells / k0 / 1e6:8.1f} GCUPS | run_dt(s_max={s_max}): {k1:10.2f} ms"
          f" {len(pairs) / k1 * 1e3:12.0f} pairs/s | run / run_dt {k0 / k1:7.3f}  (repeats {' '.join(f'{x:.2f}' for x in nw)} |"
          f" {' '.join(f'{x:.2f}' for x in dt)})", flush=True)
    print(f"{'':44s} {mname:14s} dt_info: front_cells {di['front_cells']:.4g} ({di['front_cells'] / cells:.4f} of |a||b|), extend_chars"
          f" {di['extend_chars']:.4g}, chunks {di['chunks']}, {di['bytes_max'] / 2**20:.1f} MiB, found {di['found']}, mean cost {float(want.mean()):.1f}",
          flush=True)


def double_dt_legs(title, pairs, chain, ends):
    """Affine4Batch under double_affine(4, 6, 2, 24, 1): run() and run_dt(largest cost) alternating on one batch (ends: the ends-free run()
    and run_dt_ends, both ends free); then AffineBatch.run_dt under affine(4, 6, 2) on the same pairs."""
    cm4, cm2 = AffineCost.double_affine(4, 6, 2, 24, 1), AffineCost.affine(4, 6, 2)
    cells = float(sum(len(x) * len(y) for x, y in pairs))
    b = Affine4Batch(pairs, cm4, chain=chain)
    if ends:
        b.set_free_ends(True, True)
    want = b.run()
    want_end = b.ends()[:, 1] if ends else None
    s_max = int(want.max())
    nw, dt = [], []
    for rep in range(4):  # the first round warms both routes
        c = b.run()
        k = b.last_kernel_ms
        if ends:
            d, e = b.run_dt_ends(s_max, True, True)
            same = e.tolist() == want_end.tolist()
        else:
            d, same = b.run_dt(s_max), True
        if c.tolist() != want.tolist() or d.tolist() != want.tolist() or not same:
            raise SystemExit(f"{title}: Affine4Batch.run() and run_dt() disagree")
        if rep:
            nw.append(k)
            dt.append(b.last_kernel_ms)
    di = b.dt_info()
    b.close()
    b2 = AffineBatch(pairs, cm2, chain=chain, free_start=ends, free_end=ends)
    want2 = b2.run()
    s2 = int(want2.max())
    dt2 = []
    for rep in range(4):
        d = b2.run_dt_ends(s2, True, True)[0] if ends else b2.run_dt(s2)
        if d.tolist() != want2.tolist():
            raise SystemExit(f"{title}: AffineBatch.run() and run_dt() disagree")
        if rep:
            dt2.append(b2.last_kernel_ms)
    di2 = b2.dt_info()
    b2.close()
    k0, k1, k2 = min(nw), min(dt), min(dt2)
    call = "run_dt_ends" if ends else "run_dt"
    print(f"{title:44s} double_affine  run(){' chained' if chain else ''}{' ends-free' if ends else ''}: {k0:10.2f} ms {cells / k0 / 1e6:8.1f} GCUPS |"
          f" {call}(s_max={s_max}): {k1:10.2f} ms {len(pairs) / k1 * 1e3:12.0f} pairs/s | run / {call} {k0 / k1:7.3f}"
          f"  (repeats {' '.join(f'{x:.2f}' for x in nw)} | {' '.join(f'{x:.2f}' for x in dt)})", flush=True)
    print(f"{'':44s} double_affine  dt_info: front_cells {di['front_cells']:.4g} ({di['front_cells'] / cells:.4f} of |a||b|), extend_chars"
          f" {di['extend_chars']:.4g}, chunks {di['chunks']}, {di['bytes_max'] / 2**20:.1f} MiB, found {di['found']}, mean cost {float(want.mean()):.1f}",
          flush=True)
    print(f"{'':44s} affine(4,6,2)  {call}(s_max={s2}): {k2:10.2f} ms | four-layer / two-layer DT {k1 / k2:7.3f}  (repeats"
          f" {' '.join(f'{x:.2f}' for x in dt2)}); front_cells {di2['front_cells']:.4g}, extend_chars {di2['extend_chars']:.4g},"
          f" {di2['bytes_max'] / 2**20:.1f} MiB, mean cost {float(want2.mean()):.1f}", flush=True)


def dt_seg_legs(title, pairs, cm, mname, Batch=AffineBatch):
    """align_dt_ends(largest cost) and align_dt_seg(largest cost), both switches off, in turn on one traced batch (with
    Batch = Affine4Batch the segmented call is align_dt_segmented)."""
    b = Batch(pairs, cm, trace=True)
    seg_call, seg_info = (b.align_dt_segmented, b.dt_segmented_info) if Batch is Affine4Batch else (b.align_dt_seg, b.dt_seg_info)
    s_max = int(b.run_dt((1 << 30) - 1).max())
    every, seg, err = [], [], None
    for rep in range(4):  # the first round warms both routes
        want = None
        if err is None:
            try:
                want = b.align_dt_ends(s_max, False, False)
                if rep:
                    every.append((b.last_forward_ms, b.last_trace_ms, b.dt_info()))
            except ValueError as e:
                err = str(e)
        got = seg_call(s_max, 0, False, False)
        if want is not None and got != want:
            raise SystemExit(f"{title} {mname}: align_dt_ends() and align_dt_seg() disagree")
        if any(g[0] < 0 for g in got):
            raise SystemExit(f"{title} {mname}: align_dt_seg() did not find a pair within the largest cost")
        if rep:
            seg.append((b.last_forward_ms, b.last_refill_ms, b.last_trace_ms, seg_info()))
    b.close()
    f1, r1, w1, si = min(seg, key=lambda x: sum(x[:3]))
    t1 = f1 + r1 + w1
    line = (f"align_dt_seg: forward {f1:.2f} + refill {r1:.2f} + walk {w1:.2f} = {t1:.2f} ms, rounds {si['rounds']}, chunks {si['chunks']},"
            f" {si['bytes_max'] / 2**20:.1f} MiB, seg jobs {si['seg_jobs']}, refill cells {si['refill_cells']:.4g}"
            f"  (repeats {' '.join(f'{sum(x[:3]):.2f}' for x in seg)})")
    if every:
        f0, w0, di = min(every, key=lambda x: x[0] + x[1])
        t0 = f0 + w0
        print(f"{title:44s} {mname:14s} s_max {s_max}: align_dt_ends: forward {f0:.2f} + walk {w0:.2f} = {t0:.2f} ms, chunks {di['chunks']},"
              f" {di['bytes_max'] / 2**20:.1f} MiB  (repeats {' '.join(f'{x[0] + x[1]:.2f}' for x in every)})", flush=True)
        print(f"{'':44s} {mname:14s} {line}", flush=True)
        print(f"{'':44s} {mname:14s} time seg / ends {t1 / t0:.3f} (forward {f1 / f0:.3f}), bytes_max ends / seg {di['bytes_max'] / si['bytes_max']:.1f}",
              flush=True)
    else:
        print(f"{title:44s} {mname:14s} s_max {s_max}: align_dt_ends: {err}", flush=True)
        print(f"{'':44s} {mname:14s} {line}", flush=True)


def ends_shape(name, rng, rate=0.05, offsets=None):
    """(text, pattern) pairs: a mutated piece of the window, somewhere inside it (`offsets`, a list, receives where)."""
    count, plen, wlen = (100_000, 150, 400) if name == "map150" else (4096, 10_000, 12_000)
    pairs = []
    for _ in range(count):
        w = rand_seq(rng, wlen)
        off = int(rng.integers(0, wlen - plen + 1))
        pairs.append((w, mutate(rng, w[off:off + plen], rate)))
        if offsets is not None:
            offsets.append(off)
    return f"{count} x {plen} bp in {wlen} bp windows", pairs


def dt_ends_legs(title, pairs, cm, mname, fs, fe):
    """Ends-free run() and run_dt_ends(largest cost), alternating on one batch; the cost and end of every pair must agree."""
    cells = float(sum(len(x) * len(y) for x, y in pairs))
    b = AffineBatch(pairs, cm, free_start=fs, free_end=fe)
    want = b.run()
    want_end = b.ends()[:, 1]
    s_max = int(want.max())
    nw, dt = [], []
    for rep in range(4):  # the first round warms both routes
        c = b.run()
        k = b.last_kernel_ms
        d, e = b.run_dt_ends(s_max, fs, fe)
        if c.tolist() != want.tolist() or d.tolist() != want.tolist() or e.tolist() != want_end.tolist():
            raise SystemExit(f"{title} {mname}: run() and run_dt_ends() disagree")
        if rep:
            nw.append(k)
            dt.append(b.last_kernel_ms)
    di = b.dt_info()
    b.close()
    k0, k1 = min(nw), min(dt)
    mode = "both ends free" if fs else "free_end only"
    print(f"{title:44s} {mname:14s} {mode:15s} run(): {k0:10.2f} ms {cells / k0 / 1e6:8.1f} GCUPS | run_dt_ends(s_max={s_max}): {k1:10.2f} ms"
          f" {len(pairs) / k1 * 1e3:12.0f} pairs/s | run / run_dt_ends {k0 / k1:7.3f}  (repeats {' '.join(f'{x:.2f}' for x in nw)} |"
          f" {' '.join(f'{x:.2f}' for x in dt)})", flush=True)
    print(f"{'':44s} {mname:14s} {'':15s} dt_info: front_cells {di['front_cells']:.4g} ({di['front_cells'] / cells:.4f} of |a||b|), extend_chars"
          f" {di['extend_chars']:.4g}, chunks {di['chunks']}, {di['bytes_max'] / 2**20:.1f} MiB, found {di['found']}, mean cost {float(want.mean()):.1f}",
          flush=True)


def ends_legs(title, pairs, tp, cm, mname, tile_cols, reps, Batch=AffineBatch):
    """Global and ends-free, alternating: run() on a batch of `pairs`, align() and align_tiled() on a traced batch of `tp`."""
    cells, tcells = float(sum(len(x) * len(y) for x, y in pairs)), float(sum(len(x) * len(y) for x, y in tp))
    b, tb = Batch(pairs, cm), Batch(tp, cm, trace=True)
    ms = {(leg, on): [] for leg in ("cost", "traced", "tiled") for on in (False, True)}
    inside = 0
    for rep_ in range(reps + 1):  # the first round warms every route
        for on in (False, True):
            b.set_free_ends(on, on)
            tb.set_free_ends(on, on)
            b.run()
            k = b.last_kernel_ms
            tb.align()
            u = tb.last_forward_ms + tb.last_trace_ms
            tb.align_tiled(tile_cols)
            t = tb.last_forward_ms + tb.last_refill_ms + getattr(tb, Batch._WALK_MS)
            if on:
                se = tb.ends()
                inside = int(((se[:, 0] > 0) & (se[:, 1] < np.array([len(x) for x, _ in tp]))).sum())
            if rep_:
                ms[("cost", on)].append(k)
                ms[("traced", on)].append(u)
                ms[("tiled", on)].append(t)
    ti = tb.tiled_info()
    b.close()
    tb.close()
    for leg, c, npairs in (("cost", cells, len(pairs)), ("traced", tcells, len(tp)), ("tiled", tcells, len(tp))):
        g, e = min(ms[(leg, False)]), min(ms[(leg, True)])
        print(f"{title:44s} {mname:14s} {leg + ':':10s} global {g:10.2f} ms {c / g / 1e6:8.1f} GCUPS | ends-free {e:10.2f} ms {c / e / 1e6:8.1f} GCUPS"
              f" | ends-free / global {e / g:6.3f}  ({npairs} pairs; repeats {' '.join(f'{x:.2f}' for x in ms[(leg, False)])} |"
              f" {' '.join(f'{x:.2f}' for x in ms[(leg, True)])})", flush=True)
    print(f"{'':44s} {mname:14s} ends-free: {inside} of {len(tp)} traced pairs start after column 0 and end before |a|; tiled: {ti['tile_jobs']} tile jobs,"
          f" {ti['refill_cells'] / tcells:.3f} of the cells filled", flush=True)


def local_legs(title, pairs, tp, cm, mname, match=2, Batch=AffineBatch):
    """Global and local (run_local / align_local at `match`; run_sw / align_sw of an Affine4Batch), alternating on one batch each: run()
    against run_local() on `pairs` (if any), align() against align_local() on a traced batch of `tp` (if any); each warmed once, then
    three times, the fastest of each."""
    run_local, align_local, local_info = ("run_sw", "align_sw", "sw_info") if Batch is Affine4Batch else ("run_local", "align_local", "local_info")
    legs = []
    if pairs:
        b = Batch(pairs, cm)
        g, l = [], []
        for rep in range(4):  # the first round warms both routes
            b.run()
            k = b.last_kernel_ms
            getattr(b, run_local)(match)
            if rep:
                g.append(k)
                l.append(b.last_kernel_ms)
        b.close()
        legs.append(("cost", pairs, g, l, ""))
    if tp:
        tb = Batch(tp, cm, trace=True)
        g, l, gf, lf = [], [], [], []  # totals, and the forward (fill) part of each
        for rep in range(4):
            tb.align()
            k, kf = tb.last_forward_ms + tb.last_trace_ms, tb.last_forward_ms
            res = getattr(tb, align_local)(match)
            if rep:
                g.append(k)
                gf.append(kf)
                l.append(tb.last_forward_ms + tb.last_trace_ms)
                lf.append(tb.last_forward_ms)
        li = getattr(tb, local_info)()
        tb.close()
        cover = sum(r[5] - r[4] for r in res) / max(sum(len(y) for _, y in tp), 1)
        legs.append(("traced", tp, g, l, f"; fills {min(gf):.2f} | {min(lf):.2f} ms; {li['chunks']} chunks, {li['bytes_max'] / 2**20:.0f} MiB,"
                                         f" {cover:.3f} of b aligned"))
    for leg, ps, g, l, note in legs:
        cells = float(sum(len(x) * len(y) for x, y in ps))
        g0, l0 = min(g), min(l)
        print(f"{title:44s} {mname:14s} {leg + ':':10s} global {g0:10.2f} ms {cells / g0 / 1e6:8.1f} GCUPS | local(match={match}) {l0:10.2f} ms"
              f" {cells / l0 / 1e6:8.1f} GCUPS | local / global {l0 / g0:6.3f}  ({len(ps)} pairs; repeats {' '.join(f'{x:.2f}' for x in g)} |"
              f" {' '.join(f'{x:.2f}' for x in l)}{note})", flush=True)


def traced(tp, cm, mname, untiled, tile_cols, reps, warm=True, note=""):
    """The traced lines of one batch: the untiled route (if asked for) and the tiled one, alternating."""
    tcells = float(sum(len(x) * len(y) for x, y in tp))
    tb = AffineBatch(tp, cm, trace=True)
    if warm:
        if untiled:
            tb.align()
        tb.align_tiled(tile_cols)
    u, t = [], []
    for _ in range(reps):
        if untiled:
            tb.align()
            u.append((tb.last_forward_ms, tb.last_trace_ms))
        tb.align_tiled(tile_cols)
        t.append((tb.last_forward_ms, tb.last_refill_ms, tb.last_trace_ms))
    if untiled:
        f, w = min(u, key=sum)
        print(f"{'':44s} {mname:14s} traced:    {f + w:10.2f} ms {tcells / (f + w) / 1e6:8.1f} GCUPS {len(tp) / (f + w) * 1e3:12.0f} pairs/s"
              f"  (forward {f:.2f} ms = {tcells / f / 1e6:.1f} GCUPS, walks {w:.2f} ms, {tb.info()['trace_chunks']} chunks, {len(tp)} pairs;"
              f" repeats {' '.join(f'{sum(x):.2f}' for x in u)})", flush=True)
    f, r, w = min(t, key=sum)
    ti = tb.tiled_info()
    print(f"{'':44s} {mname:14s} traced (tiled):{f + r + w:7.2f} ms {tcells / (f + r + w) / 1e6:8.1f} GCUPS {len(tp) / (f + r + w) * 1e3:12.0f} pairs/s"
          f"  (forward {f:.2f} ms, fills {r:.2f} ms, walks {w:.2f} ms, {ti['chunks']} chunks, {ti['rounds']} rounds, {ti['tile_jobs']} tile jobs,"
          f" {ti['refill_cells'] / tcells:.3f} of the cells filled, {ti['chunk_bytes_max'] / 2**20:.1f} MiB, {len(tp)} pairs{note};"
          f" repeats {' '.join(f'{sum(x):.2f}' for x in t)})", flush=True)
    tb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reads,10k,100k")
    ap.add_argument("--trace-100k", action="store_true", help="also trace the 100 kbp pairs untiled (10 GB of codes each)")
    ap.add_argument("--tile-cols", type=int, default=0, help="columns of a tile of the tiled route (0: the library's default)")
    ap.add_argument("--reps", type=int, default=3, help="timed repeats of each traced route")
    ap.add_argument("--trace-pairs", type=int, default=512, help="traced runs of the 10 kbp shape use this many of its pairs")
    ap.add_argument("--chain", action="store_true", help="measure the chained route against the unchained one instead (see above)")
    ap.add_argument("--ends", action="store_true", help="measure the ends-free mode against the global one instead (see above)")
    ap.add_argument("--local", action="store_true", help="measure local alignment (run_local / align_local) against the global calls instead (see above)")
    ap.add_argument("--double-local", action="store_true", help="measure Affine4Batch.run_sw / align_sw against its global calls instead (see above)")
    ap.add_argument("--dt", action="store_true", help="measure the diagonal-transition route against run() instead (see above)")
    ap.add_argument("--dt-ends", action="store_true", help="measure the ends-free diagonal-transition route against the ends-free run() instead (see above)")
    ap.add_argument("--dt-seg", action="store_true", help="measure the segmented DT traceback against align_dt_ends instead (see above)")
    ap.add_argument("--double", action="store_true", help="measure Affine4Batch under double_affine against AffineBatch under affine instead (see above)")
    ap.add_argument("--double-tiled", action="store_true", help="measure Affine4Batch.align_tiled() against Affine4Batch.align() instead (see above)")
    ap.add_argument("--double-tiled-100k", action="store_true", help=argparse.SUPPRESS)  # the 100 kbp leg of --double-tiled, in a process of its own
    ap.add_argument("--double-chain", action="store_true", help="measure Affine4Batch's chained route against its unchained one instead (see above)")
    ap.add_argument("--double-chain-shape", default="", help=argparse.SUPPRESS)  # one shape of --double-chain, in a process of its own
    ap.add_argument("--double-ends", action="store_true", help="measure Affine4Batch's ends-free mode against its global one instead (see above)")
    ap.add_argument("--double-dt", action="store_true", help="measure Affine4Batch.run_dt() against Affine4Batch.run() instead (see above)")
    ap.add_argument("--double-dt-ends", action="store_true", help="measure Affine4Batch.run_dt_ends() against the ends-free Affine4Batch.run() instead (see above)")
    ap.add_argument("--double-dt-seg", action="store_true", help="measure Affine4Batch.align_dt_segmented() against Affine4Batch.align_dt_ends() instead (see above)")
    ap.add_argument("--models", default="affine,unit", help="cost models to run: affine (affine(4, 6, 2)), unit")
    ap.add_argument("--cpu-seconds", type=float, default=2.0, help="time spent on the CPU core per shape and model")
    args = ap.parse_args()
    pa.require_gpu()
    L = cpu_lib()
    rng = np.random.default_rng(1)
    models = {"affine(4,6,2)": AffineCost.affine(4, 6, 2), "unit()": AffineCost.unit()}
    models = {k: v for k, v in models.items() if k.split("(")[0] in args.models.split(",")}
    if args.double_chain_shape:
        rng = np.random.default_rng(2)
        title, pairs = shape(args.double_chain_shape, rng)
        chain_legs(title + ", indels in a quarter", long_indels(rng, pairs), AffineCost.double_affine(4, 6, 2, 24, 1), "double_affine", args.tile_cols,
                   args.reps, Affine4Batch)
        return
    if args.double_chain:
        for sname in DOUBLE_CHAIN_SHAPES:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--double-chain-shape", sname, "--tile-cols", str(args.tile_cols), "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=double_chain_limit_s(args.reps)).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{sname}: no result within {double_chain_limit_s(args.reps):.0f} s")
            if rc:  # (nothing more is started after a failure)
                raise SystemExit(rc)
        return
    if args.double_tiled_100k:
        title, pairs = shape("100k", np.random.default_rng(2))
        t = double_tiled_leg(title + ", indels of 20-200 bp in a quarter", long_indels(rng, pairs), False, args.tile_cols, warm=False, reps=1)
        if t > DOUBLE_100K_LIMIT_S * 1e3:
            raise SystemExit(f"{title}: {t / 1e3:.1f} s is over the limit of {DOUBLE_100K_LIMIT_S:.1f} s (two lone-wavefront passes)")
        return
    if args.double_tiled:
        long_indels(rng, shape("reads", rng)[1])  # (the pairs of --double: its 10 kbp shape comes after its reads)
        title, pairs = shape("10k", rng)
        pairs = long_indels(rng, pairs)
        title += ", indels of 20-200 bp in a quarter"
        double_tiled_leg(title, pairs[: args.trace_pairs], True, args.tile_cols)
        double_tiled_leg(title, pairs, False, args.tile_cols)
        # a process of its own under a wall-clock limit: the pairs (a minute of Python at most) and the one un-warmed call
        cmd = [sys.executable, str(Path(__file__).resolve()), "--double-tiled-100k", "--tile-cols", str(args.tile_cols)]
        try:
            rc = subprocess.run(cmd, timeout=60 + DOUBLE_100K_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"16 x 100 kbp: no result within {60 + DOUBLE_100K_LIMIT_S:.0f} s")
        if rc:
            raise SystemExit(rc)
        return
    if args.double:
        for sname in ("reads", "10k"):
            title, pairs = shape(sname, rng)
            pairs = long_indels(rng, pairs)
            double_legs(title + ", indels of 20-200 bp in a quarter", pairs, None if sname == "reads" else pairs[: args.trace_pairs])
        return
    if args.double_dt:
        for sname in [x for x in args.shapes.split(",") if "@" in x] or ["reads@5", "10k@1", "10k@3", "10k@5", "10k@8", "100k@5"]:
            title, pairs = shape(sname, rng)
            if "at 5 %" not in title and sname.endswith("@5"):
                title += " at 5 %"
            double_dt_legs(title, pairs, sname.startswith("100k"), False)
        return
    if args.double_dt_seg:
        for sname in [x for x in args.shapes.split(",") if "@" in x] or ["10k@1", "10k@3", "10k@5", "reads@5", "100k@5"]:
            title, pairs = shape(sname, rng)
            if "at 5 %" not in title and sname.endswith("@5"):
                title += " at 5 %"
            dt_seg_legs(title, pairs, AffineCost.double_affine(4, 6, 2, 24, 1), "double_affine", Affine4Batch)
        return
    if args.double_dt_ends:
        for sname in [x for x in args.shapes.split(",") if x.startswith("map")] or ["map150", "map10k@1", "map10k@3", "map10k@5"]:
            name, _, pct = sname.partition("@")
            title, pairs = ends_shape(name, rng, float(pct or 5) / 100)
            double_dt_legs(f"{title} at {pct or 5} %", pairs, False, True)
        return
    if args.double_ends:
        for sname in ("map150", "map10k"):
            title, pairs = ends_shape(sname, rng)
            ends_legs(title, pairs, pairs if sname == "map150" else pairs[: args.trace_pairs], AffineCost.double_affine(4, 6, 2, 24, 1), "double_affine",
                      args.tile_cols, args.reps, Affine4Batch)
        return
    if args.double_local:
        cm4 = AffineCost.double_affine(4, 6, 2, 24, 1)
        title, pairs = ends_shape("map150", rng)
        local_legs(title, pairs, pairs, cm4, "double_affine", Batch=Affine4Batch)
        title, pairs = shape("10k", rng)
        local_legs(title, pairs, pairs[: args.trace_pairs], cm4, "double_affine", Batch=Affine4Batch)
        return
    if args.local:
        title, pairs = ends_shape("map150", rng)
        for mname, cm in models.items():
            local_legs(title, pairs, pairs, cm, mname)
        title, pairs = shape("10k", rng)
        for mname, cm in models.items():
            local_legs(title, pairs, pairs[: args.trace_pairs], cm, mname)
        return
    if args.ends:
        for sname in ("map150", "map10k"):
            title, pairs = ends_shape(sname, rng)
            for mname, cm in models.items():
                ends_legs(title, pairs, pairs if sname == "map150" else pairs[: args.trace_pairs], cm, mname, args.tile_cols, args.reps)
        return
    if args.dt_ends:
        own = [s for s in args.shapes.split(",") if s.startswith("map")] or ["map150", "map10k@1", "map10k@3", "map10k@5"]
        for sname in own:
            name, _, pct = sname.partition("@")
            offs = []
            title, pairs = ends_shape(name, rng, float(pct or 5) / 100, offs)
            seeded = [(w[o:], y) for (w, y), o in zip(pairs, offs)]  # extension: the text begins where the pattern does
            for mname, cm in models.items():
                dt_ends_legs(f"{title} at {pct or 5} %", pairs, cm, mname, True, True)
                dt_ends_legs(f"{title} at {pct or 5} %, from the seed", seeded, cm, mname, False, True)
        return
    for sname in args.shapes.split(","):
        title, pairs = shape(sname, rng)
        cells = float(sum(len(x) * len(y) for x, y in pairs))
        for mname, cm in models.items():
            if args.dt:
                dt_legs(title, pairs, cm, mname, sname.startswith("100k"))
                continue
            if args.dt_seg:
                dt_seg_legs(title, pairs, cm, mname)
                continue
            if args.chain:
                chain_legs(title, pairs, cm, mname, args.tile_cols, args.reps)
                continue
            trace = not sname.startswith("100k") or args.trace_100k
            b = AffineBatch(pairs, cm)
            info = b.info()
            b.run()  # warm-up
            ms = []
            for _ in range(3):
                b.run()
                ms.append(b.last_kernel_ms)
            k = min(ms)
            line = (f"{title:44s} {mname:14s} cost-only: {k:10.2f} ms {cells / k / 1e6:8.1f} GCUPS {len(pairs) / k * 1e3:12.0f} pairs/s"
                    f"  (waves {info['waves']}, lane use {info['lane_use']:.3f})")
            print(line, flush=True)
            b.close()
            if sname == "10k":
                traced(pairs[: args.trace_pairs], cm, mname, True, args.tile_cols, args.reps)
                traced(pairs, cm, mname, False, args.tile_cols, args.reps)
            elif sname.startswith("100k"):
                if not trace:
                    print(f"{'':44s} {mname:14s} traced:    not measured", flush=True)
                traced(pairs, cm, mname, trace, args.tile_cols, 1, warm=False, note=", unwarmed")
            else:
                traced(pairs, cm, mname, True, args.tile_cols, args.reps)
            if L is not None:
                done, c0, t0 = 0, 0.0, time.perf_counter()
                for x, y in pairs:
                    L.gotoh(x, len(x), y, len(y), *cpu_args(cm))
                    done += 1
                    c0 += len(x) * len(y)
                    if time.perf_counter() - t0 > args.cpu_seconds:
                        break
                dt = time.perf_counter() - t0
                print(f"{'':44s} {mname:14s} CPU core:  {c0 / dt / 1e9:8.3f} GCUPS {done / dt:12.1f} pairs/s  ({done} pairs, scalar Gotoh, cc -O3)",
                      flush=True)


if __name__ == "__main__":
    main()
