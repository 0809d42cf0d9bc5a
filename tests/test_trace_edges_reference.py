"""The inputs of tests/test_gpu_trace_edges.py, pinned on the CPU.

For every constructed pair and option set of tests/trace_edges.py the second restatement (oracle/astarpa2_restated.py) equals
`oracle.cpu_align` -- csrc/engine.hpp over the CPU kernels, the host code the traceback kernel was transcribed from -- in cost, CIGAR
string and the six trace statistics, in both option families (full-DP traced batch, A*PA2 batch of the `simple` family), and passes the
plain checks of trace_edges.reference (plain Levenshtein DP, plain CIGAR walk, no repeated op).  A mismatch on the GPU is then the
kernel's.  And every edge the pairs were built for shows in the restatement's statistics, so that the GPU test cannot pass by never
reaching it: DT successes and fallbacks in every cell of the option grid, blocks that end at level L = 30 .. 40 (max_g itself included)
on diagonal +-L, re-fills of 1 .. 4 strips whose tallest one is exactly ceil(m / 64) words, 128 at m = 8192 and 129 at m = 8193."""
import pytest

from tests import trace_edges as te
from tests.test_restated_engine import BASE


def engine_params(o, opts):
    d = dict(domain="astar", dt_trace=True, max_g=40, fr_drop=10)
    d.update(opts)
    front = dict(dt_trace=d["dt_trace"], max_g=d["max_g"], fr_drop=d["fr_drop"])
    if d["domain"] == "full":
        return o.make_params(domain="full", heuristic="none", doubling="none", block_width=256, sparse=True, incremental_doubling=False, **front)
    return o.make_params(**{**BASE, "heuristic": "gap", **front})


def tied(o, pairs, kw):
    """Restatement == engine over the CPU kernels for every pair, both families -> {family name: [statistics per pair]}."""
    out = {}
    for name, fam in (("full", te.FULL), ("gap", te.GAP)):
        opts = {**fam, **kw}
        prm = engine_params(o, opts)
        out[name] = []
        for a, b in pairs:
            cost, cigar, stats = te.reference(a, b, opts)
            w_cost, w_cigar, w_stats = o.cpu_align(a, b, prm)
            assert (cost, cigar) == (w_cost, w_cigar), (name, kw, len(a), len(b), cigar[:60], w_cigar[:60])
            assert te.trace_stats(stats) == te.trace_stats(w_stats), (name, kw, len(a), len(b))
            assert sum(te.trace_stats(stats)[1:3]) == stats["dt_trace_tries"] and sum(te.trace_stats(stats)[4:]) == stats["fill_tries"]
            assert len(a) <= 1100 and len(b) <= 8300
            out[name].append(stats)
    return out


def total(stats, key):
    return sum(s[key] for s in stats)


@pytest.mark.parametrize("max_g", te.GRID_MAX_G)
def test_option_grid(oracle, max_g):
    twelve = te.grid_long_pairs()
    assert len(twelve) == 12 and len(te.grid_pairs()) == 17
    fb = {}
    for fr_drop in te.GRID_FR_DROP:
        kw = te.dt_kw(max_g, fr_drop)
        for name, stats in tied(oracle, te.grid_pairs(), kw).items():
            long_stats = stats[:12]
            # every cell decides both ways, over the twelve pairs of 258 .. 1025 bases alone
            assert total(long_stats, "dt_trace_success") >= 1 and total(long_stats, "dt_trace_fallback") >= 1, (name, kw)
            assert all(s["max_fill_words"] <= te.SCRATCH_WORDS for s in stats)
            fb[name, fr_drop] = (total(long_stats, "dt_trace_success"), total(long_stats, "dt_trace_fallback"))
            assert stats[12]["dt_trace_tries"] == 0  # n = 1: a block of one column is never tried
    if max_g == 1:
        assert fb["full", 0] == (4, 29)
    if max_g == 40:
        assert fb["full", 0] == fb["full", 1000] == (25, 8) and fb["full", 1] == (23, 10)  # (a narrow x-drop loses two blocks)


def test_single_column_blocks_are_not_tried(oracle):
    """n = 257, 513: the last block is one column next to a checkpoint -- no DT (`i0 < to_i - 1` fails) and no re-fill for it; n = 258: two
    columns, DT runs."""
    for kw in (te.dt_kw(40, 10), te.NO_DT):
        for (label, a, b), blocks_tried in zip(te.last_column_pairs(), (1, 2, 2)):
            n = len(a)
            s = te.reference(a, b, {**te.FULL, **kw})[2]
            if kw["dt_trace"]:
                assert te.trace_stats(s) == [blocks_tried, blocks_tried, 0, 0, 0, 0], (n, s)
            else:
                assert te.trace_stats(s) == [0, 0, 0, blocks_tried, blocks_tried, 0], (n, s)


@pytest.mark.parametrize("fr_drop", te.WIDE_DROPS)
def test_wide_levels(oracle, fr_drop):
    cases = te.wide_pairs()
    assert len(cases) == 16
    got = tied(oracle, [(a, b) for _, _, a, b in cases], te.dt_kw(40, fr_drop))
    for name, stats in got.items():
        for (L, kind, a, b), s in zip(cases, stats):
            cost, cigar, _ = te.reference(a, b, {**(te.FULL if name == "full" else te.GAP), **te.dt_kw(40, fr_drop)})
            assert cost == L and abs(len(a) - len(b)) == L, (L, kind)
            # L indels of one sign and nothing else, all inside the second block: that block ends at level L (2 L + 1 diagonals: more
            # than a wavefront from L = 32) on diagonal +-L, the other two at level 0
            i, cols = 0, []
            for k, op in te.cigar_elems(cigar):
                assert op != "X"
                if op in "ID":
                    cols.append(i)
                i += k if op != "I" else 0
            assert 256 < min(cols) and max(cols) < 512 and len(a) > 512, (L, kind, cigar)
            if fr_drop == 10:  # the preset's x-drop gives that block up
                assert te.trace_stats(s)[:3] == [2, 1, 1], (name, L, kind, s)
            else:              # every block by DT, L = 40 at exactly max_g
                assert te.trace_stats(s) == [3, 3, 0, 0, 0, 0], (name, L, kind, s)


def test_wide_levels_fail_one_past_max_g(oracle):
    """max_g reached exactly: the L = 40 pairs succeed at max_g = 40 and fall back at 39."""
    cases = [(a, b) for L, _, a, b in te.wide_pairs() if L == 40]
    for stats in tied(oracle, cases, te.dt_kw(39, 0)).values():
        assert all(s["dt_trace_fallback"] == 1 and s["fill_success"] == 1 for s in stats), stats


@pytest.mark.parametrize("kw", te.EXT_KWS, ids=lambda k: "g{max_g}_drop{fr_drop}".format(**k) if k["dt_trace"] else "no_dt")
def test_extension_edges(oracle, kw):
    cases = te.extension_pairs()
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels)
    got = tied(oracle, [(a, b) for _, a, b in cases], kw)
    for name, stats in got.items():
        by = dict(zip(labels, stats))
        fam = te.FULL if name == "full" else te.GAP
        for (label, a, b), s in zip(cases, stats):
            cost, cigar, _ = te.reference(a, b, {**fam, **kw})
            if label.startswith("identical"):
                assert cigar == f"{len(a)}=" and s["dt_trace_fallback"] == 0
            if label.startswith(("sub_run", "ins_run", "del_run")):
                assert cost == 2
                if kw["dt_trace"]:  # two edits in one block: by DT from max_g = 2 on (success AT max_g), re-filled at max_g = 1
                    assert (s["dt_trace_fallback"] == 0) == (kw["max_g"] >= 2), (label, kw, s)
            if label.startswith("sub_run"):
                r = int(label[len("sub_run"):label.index("_at")])
                assert f"X{r}=X" in cigar.replace("X1=", "X="), (label, cigar)
            if label.startswith("sub_after"):
                r, off = int(label[len("sub_after"):label.index("_from")]), int(label[label.index("_from") + 5:])
                assert cigar == f"{off + r}=X39=" and (not kw["dt_trace"] or s["dt_trace_fallback"] == 0)
        assert te.reference(b"A" * 300, b"A" * 290, {**fam, **kw})[:2] == (10, "10D290=")
        assert te.reference(b"A" * 300, b"A" * 310, {**fam, **kw})[:2] == (10, "10I300=")
        if kw["dt_trace"]:  # 300 columns against a handful of rows: the first-tried block cannot be done in max_g edits
            assert all(by[f"clamp_{r}rows"]["dt_trace_fallback"] >= 1 for r in (3, 40, 41))


@pytest.mark.parametrize("kw", te.REFILL_KWS, ids=["no_dt", "dt"])
@pytest.mark.parametrize("base", [2048, 4096, 6144, 8192])
def test_refill_strips_and_scratch_limit(oracle, base, kw):
    ms = [m for m in te.REFILL_M if abs(m - base) <= 64]
    assert len(ms) == 5
    tail = [te.refill_tail_pair(m) for m in ms]
    mid = [te.refill_mid_pair(m) for m in ms]
    assert all(len(b) == m for m, (_, b) in zip(ms + ms, tail + mid))
    got = tied(oracle, tail + mid + [te.ORDINARY], kw)
    for m, (a, b), s in zip(ms, tail, got["full"]):
        cost, cigar, _ = te.reference(a, b, {**te.FULL, **kw})
        assert (cost, cigar) == (m - 700, f"700=40X{m - 740}I")
        # the last block's re-fill doubles from 320 rows until it spans all of b: 1 .. 4 strips of 32 words, and the scratch limit between
        # m = 8192 (128 words) and m = 8193
        assert s["max_fill_words"] == (m + 63) // 64 and s["fill_fallback"] >= 3
        if m in (8192, 8193):
            assert (s["fill_tries"], s["fill_fallback"]) == (6, 5)
    for m, (a, b), s in zip(ms, mid, got["full"][5:]):
        assert te.reference(a, b, {**te.FULL, **kw})[:2] == (m - 700, f"300={m - 700}I400=")
        assert s["fill_fallback"] >= 3
    for name, fam in (("full", te.FULL), ("gap", te.GAP)):
        # which pairs the kernel must hand to the host engine: the tail pairs of more than 8192 rows through the full-DP batch.  (In the
        # banded blocks of the A*PA2 batch the same re-fill stops at the previous block's first row, two words short of the top; the
        # run in mid-block is re-filled from the checkpoint column at 512, 188 rows short of the end.)
        want = sum(m > 8192 for m in ms) if name == "full" else 0
        assert te.host_pairs(tail, {**fam, **kw}) == want and te.host_pairs(mid + [te.ORDINARY], {**fam, **kw}) == 0
        assert all(s["max_fill_words"] <= te.SCRATCH_WORDS for (_, b), s in zip(tail + mid, got[name]) if len(b) <= 8192)


def test_plain_checks_reject_wrong_answers():
    """The helper's own checks are not vacuous."""
    a, b = b"ACGTACGT", b"ACGAACGTT"
    assert te.levenshtein(a, b) == te.levenshtein(b, a) == 2 and te.levenshtein(b"AAAA", b"A") == 3
    assert te.cigar_cost("3=X4=I", a, b) == 2
    for bad in ("3=X3=I", "4=4=I", "3=X4=D", "8=I", "3=X2=2=I"):
        with pytest.raises(AssertionError):
            te.cigar_cost(bad, a, b)
