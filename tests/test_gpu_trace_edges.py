"""The batched traceback kernel (csrc/trace_kernel.hpp, the four trace_kernel<DT, BANDED> instances) at its DT-trace and re-fill edges,
against the second restatement of the reference's host logic (oracle/astarpa2_restated.py through tests/trace_edges.reference, which also
checks every answer against a plain Levenshtein DP and a plain CIGAR walk).  tests/test_trace_edges_reference.py pins the same inputs on
the CPU: there the restatement equals csrc/engine.hpp over the CPU kernels on every pair, and every edge the pairs were built for shows in
its statistics -- so a mismatch here is the kernel's, and the kernel cannot pass by not reaching an edge.

Every case goes through two batches: the full-DP traced batch (pa_batch_create_trace_params: instances <DT, false>) and an A*PA2 batch of
the `simple` family (GapCost, banded blocks: instances <DT, true>), whose six trace statistics per pair are compared as well.  Every
comparison is exact (cost, CIGAR string, statistics).  pa_batch_trace_fallbacks is asserted for every batch -- 0 unless the case says
otherwise; it sums over the alignment calls of a plan --, and each batch is aligned twice with equal results.

What the cases reach in the kernel:
  option grid      max_g 1 .. 40 x fr_drop 0 .. 1000 on 258 .. 1025 bases at 2 .. 20 %: the midpoint early-out at odd and tiny max_g
                   (max_g = 1: "level 0"), max_g reached, the x-drop from both ends, blocks of one and two columns
  wide levels      blocks that end at level 30 .. 40 on diagonal +-L: levels of more than 64 diagonals (the second round of lanes, a
                   success found there), the scalar x-drop loop (fr_drop = 1000), max_g reached exactly (L = 40) and missed by one
  extension edges  match runs of 7 .. 512 that end at the checkpoint column, at row 0 or at an edit: the eight-per-round routine, the
                   64-per-round one and the hand-over between them; homopolymers; 300 columns against 3 .. 41 rows (b_lo clamped at 0)
  re-fill strips   one vertical run that brings b to 2048 / 4096 / 6144 / 8192 rows -64, -1, 0, +1, +64: re-fills of 1 .. 4 strips by height
                   doubling, exactly 128 words on the GPU, 129 words handed to the host engine"""
import pytest

from tests import restated_fixture as rf
from tests import trace_edges as te

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


def run_both(pa, pairs, kw, full_host=0, gap_host=0):
    """`pairs` under the trace options `kw` through the full-DP traced batch and the A*PA2 batch; full_host / gap_host: the pairs each
    of them has to hand to the host engine."""
    for fam, host in ((te.FULL, full_host), (te.GAP, gap_host)):
        opts = {**fam, **kw}
        name = "full-DP" if fam is te.FULL else "A*PA2"
        want = [te.reference(a, b, opts) for a, b in pairs]
        prm = rf.params_from_kwargs(pa, opts)
        bt = pa.Batch(pairs, trace=True, trace_params=prm) if fam is te.FULL else pa.Batch(pairs, params=prm)
        try:
            for rep in (1, 2):
                costs, cigars, _, _ = bt.align()
                bad = [i for i, w in enumerate(want) if (int(costs[i]), cigars[i]) != w[:2]]
                assert not bad, (name, kw, rep, bad[:8], [(len(pairs[i][0]), len(pairs[i][1]), int(costs[i]), cigars[i][:60], want[i][0], want[i][1][:60])
                                                          for i in bad[:3]])
                if fam is te.GAP:
                    stats = bt.pair_stats()
                    bad = [i for i, w in enumerate(want) if te.trace_stats(stats[i]) != te.trace_stats(w[2])]
                    assert not bad, (name, kw, rep, bad[:8], [(len(pairs[i][0]), len(pairs[i][1]), te.trace_stats(stats[i]), te.trace_stats(want[i][2]))
                                                              for i in bad[:3]])
                assert bt.trace_fallbacks() == rep * host, (name, kw, rep, bt.trace_fallbacks(), host)
        finally:
            bt.close()


@pytest.mark.parametrize("max_g", te.GRID_MAX_G)
def test_option_grid(pa, max_g):
    pairs = te.grid_pairs()
    for fr_drop in te.GRID_FR_DROP:
        run_both(pa, pairs, te.dt_kw(max_g, fr_drop))


@pytest.mark.parametrize("fr_drop", te.WIDE_DROPS)
def test_wide_levels(pa, fr_drop):
    pairs = [(a, b) for _, _, a, b in te.wide_pairs()]
    run_both(pa, pairs, te.dt_kw(40, fr_drop))


def test_wide_levels_fail_one_past_max_g(pa):
    run_both(pa, [(a, b) for L, _, a, b in te.wide_pairs() if L == 40], te.dt_kw(39, 0))


@pytest.mark.parametrize("kw", te.EXT_KWS, ids=lambda k: "g{max_g}_drop{fr_drop}".format(**k) if k["dt_trace"] else "no_dt")
def test_extension_edges(pa, kw):
    run_both(pa, [(a, b) for _, a, b in te.extension_pairs()], kw)


@pytest.mark.parametrize("kw", te.REFILL_KWS, ids=["no_dt", "dt"])
@pytest.mark.parametrize("base", [2048, 4096, 6144, 8192])
def test_refill_strips_and_scratch_limit(pa, base, kw):
    ms = [m for m in te.REFILL_M if abs(m - base) <= 64]
    on_gpu = [te.refill_tail_pair(m) for m in ms if m <= 8192] + [te.refill_mid_pair(m) for m in ms] + [te.ORDINARY]
    # no pair of up to 8192 rows leaves the GPU, whatever its indel (nor the taller ones with the run in mid-block: their re-fill starts at
    # the checkpoint column at 512, 188 rows short of the end of b, and is 127 words at most)
    run_both(pa, on_gpu, kw)
    for m in ms:
        if m > 8192:
            # 129 words: more than the full-DP batch's scratch holds -- that pair alone goes to the host engine, its neighbour does not.
            # (The A*PA2 batch's banded blocks start two words down: its re-fill of this pair is 127 words and stays.)
            run_both(pa, [te.refill_tail_pair(m), te.ORDINARY], kw, full_host=1, gap_host=0)
