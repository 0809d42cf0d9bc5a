"""Inputs and reference of the edge tests of the batched traceback kernel (csrc/trace_kernel.hpp): tests/test_trace_edges_reference.py pins
them on the CPU, tests/test_gpu_trace_edges.py runs them through the four trace_kernel<DT, BANDED> instances.

The pairs are built for the kernel's own branches: DT levels wider than one wavefront (81 diagonals at max_g = 40), the two left-extension
routines with their limits at the checkpoint column and at row 0, value_at with b_lo clamped, the midpoint and max_g early-outs at odd and
tiny max_g, blocks of one and two columns, re-fills of 1 .. 4 strips and the 128-word scratch limit.

reference(a, b, kw) is the SECOND restatement of the reference's host logic (oracle/astarpa2_restated.py: pure Python on big integers, no
line shared with csrc/engine.hpp or any kernel) after three checks that depend on nothing of the project's: the cost equals a plain
Levenshtein DP (numpy rows), the CIGAR priced by a plain walk over a and b consumes both exactly and costs that much, and no two adjacent
CIGAR elements have the same op.  Results are cached: the CPU test and both batch kinds of the GPU test share one computation per
(pair, options), and nobody changes what comes back.

Two option families per case: FULL is what the full-DP traced batch (pa_batch_create_trace_params) restates, GAP the `simple` family of
the A*PA2 batch (Domain::Astar, GapCost, band doubling: banded blocks)."""
import re

import numpy as np

from oracle import astarpa2_restated as restated
from tests.util_seq import gen_pair, rand_seq

TRACE_KEYS = ["dt_trace_tries", "dt_trace_success", "dt_trace_fallback", "fill_tries", "fill_success", "fill_fallback"]
FULL = dict(domain="full", doubling="none", sparse=True)
GAP = dict(heuristic="gap")
SCRATCH_WORDS = 128  # kTraceScratchWords: a re-fill of more 64-row words than this goes to the host engine


# ---- the plain checks ----
def levenshtein(a: bytes, b: bytes) -> int:
    """Unit-cost edit distance, one numpy row per character of the shorter sequence."""
    if len(a) > len(b):
        a, b = b, a
    B = np.frombuffer(b, np.uint8)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    row = idx.copy()
    for i, ch in enumerate(a, 1):
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[1:] + 1, row[:-1] + (B != ch))
        row = np.minimum.accumulate(new - idx) + idx  # new[j] = min over k <= j of new[k] + (j - k)
    return int(row[-1])


_ELEM = re.compile(r"(\d*)([=XID])")


def cigar_elems(cigar: str):
    pos, out = 0, []
    for mt in _ELEM.finditer(cigar):
        assert mt.start() == pos, f"bad CIGAR {cigar!r}"
        pos = mt.end()
        out.append((int(mt.group(1) or 1), mt.group(2)))
    assert pos == len(cigar), f"bad CIGAR {cigar!r}"
    return out


def cigar_cost(cigar: str, a: bytes, b: bytes) -> int:
    """Unit-cost price of a CIGAR by a plain walk: '=' on equal bytes, 'X' on different ones, 'I' advances b, 'D' advances a; both
    sequences consumed exactly; adjacent elements differ in their op."""
    i = j = cost = 0
    last = None
    for k, op in cigar_elems(cigar):
        assert k >= 1 and op != last, f"empty or repeated element in {cigar[:80]!r}"
        last = op
        if op in "=X":
            assert i + k <= len(a) and j + k <= len(b), "CIGAR runs past a sequence"
            same = [a[i + t] == b[j + t] for t in range(k)]
            assert all(same) if op == "=" else not any(same), f"{k}{op} at ({i}, {j})"
            i, j = i + k, j + k
        elif op == "I":
            j += k
        else:
            i += k
        cost += 0 if op == "=" else k
    assert (i, j) == (len(a), len(b)), f"CIGAR consumes ({i}, {j}) of ({len(a)}, {len(b)})"
    return cost


class _Counting(restated.Restated):
    """The restatement, noting the tallest re-fill it makes (in 64-row words): what the kernel's scratch has to hold."""
    max_fill_words = 0

    def fill_with_blocks(self, i_range, original_j_range):
        self.max_fill_words = max(self.max_fill_words, (original_j_range[1] - original_j_range[0] + 63) // 64)
        return super().fill_with_blocks(i_range, original_j_range)


_lev, _ref = {}, {}


def reference(a: bytes, b: bytes, kw: dict):
    """-> (cost, CIGAR string, statistics) of the restatement for restated.align's keyword arguments, after the plain checks.  The
    statistics carry one more entry, `max_fill_words`: the tallest re-fill of the trace in words."""
    key = (a, b, tuple(sorted(kw.items())))
    if key not in _ref:
        r = _Counting(a, b, **kw)
        cost, cigar, stats = r.align()
        if (a, b) not in _lev:
            _lev[(a, b)] = levenshtein(a, b)
        assert cost == _lev[(a, b)], (len(a), len(b), kw, cost, _lev[(a, b)])
        assert cigar_cost(cigar, a, b) == cost, (len(a), len(b), kw)
        _ref[key] = (cost, cigar, dict(stats, max_fill_words=r.max_fill_words))
    return _ref[key]


def host_pairs(pairs, kw: dict) -> int:
    """How many of the pairs the kernel has to hand to the host engine: those with a re-fill taller than its scratch."""
    return sum(reference(a, b, kw)[2]["max_fill_words"] > SCRATCH_WORDS for a, b in pairs)


def trace_stats(stats) -> list:
    return [int(stats[k]) for k in TRACE_KEYS]


# ---- (a) the option grid ----
GRID_MAX_G = [1, 2, 3, 5, 20, 39, 40]
GRID_FR_DROP = [0, 1, 10, 20, 1000]
GRID_CELLS = [(g, d) for g in GRID_MAX_G for d in GRID_FR_DROP]


def dt_kw(max_g: int, fr_drop: int) -> dict:
    return dict(dt_trace=True, max_g=max_g, fr_drop=fr_drop)


NO_DT = dict(dt_trace=False)


def grid_long_pairs():
    """Twelve pairs over 2 .. 5 blocks: two columns left in the last block (258), one (513, 769, 1025)."""
    return [gen_pair(n, e, seed=n * 13 + int(100 * e)) for n in (258, 513, 769, 1025) for e in (0.02, 0.08, 0.2)]


def grid_boundary_pairs():
    """The block-boundary sizes; at 20 % so that even the 255 .. 257 ones carry a few dozen edits."""
    return [gen_pair(n, 0.2, seed=n * 13 + 20) for n in (1, 2, 255, 256, 257)]


def grid_pairs():
    return grid_long_pairs() + grid_boundary_pairs()


# ---- (b) levels wider than 64 diagonals ----
WIDE_L = [30, 33, 36, 40]
WIDE_DROPS = [0, 1000, 10]  # no x-drop, one that never prunes (the scalar loop from level 32 on), the preset's as the contrast


def wide_pairs():
    """One indel of L bases at column 300 of 600, as a deletion and as an insertion, each also swapped: the block that holds it ends at
    level L on diagonal +-L.  -> [(L, kind, a, b)]"""
    a = rand_seq(600, seed=3)
    out = []
    for L in WIDE_L:
        dl = a[:300] + a[300 + L:]
        ins = a[:300] + rand_seq(L, seed=9) + a[300:]
        out += [(L, "del", a, dl), (L, "del_swapped", dl, a), (L, "ins", a, ins), (L, "ins_swapped", ins, a)]
    return out


# ---- (c) extension edges ----
IDENT_N = [7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512]
RUN_N = [7, 8, 9, 15, 16, 17, 63, 64, 65, 200]


def other_base(c: int) -> bytes:
    return b"A" if c != ord("A") else b"C"


def last_column_pairs():
    """One substitution per block, the last block's in its last column: at n = 257 and 513 that block is a single column (walked as
    stored, neither DT nor a re-fill), at 258 it has two (the smallest DT runs on).  -> [(label, a, b)]"""
    out = []
    for n in (257, 258, 513):
        a = rand_seq(n, seed=n)
        b = bytearray(a)
        for q in (100, 300, n - 1):
            if q < n:
                b[q:q + 1] = other_base(a[q])
        out.append((f"last_column{n}", a, bytes(b)))
    return out


def extension_pairs():
    """-> [(label, a, b)]"""
    out = [(f"identical{n}", s, s) for n in IDENT_N for s in [rand_seq(n, seed=100 + n)]] + last_column_pairs()
    for r in RUN_N:
        # exactly r matching bases between a substitution at column 20 of a block and a second edit r + 1 columns to its right, in the first
        # block and in the second (whose left edge is a checkpoint column, not column 0); with an indel as the second edit several
        # diagonals are alive when the run starts
        for off in (0, 256):
            s = rand_seq(off + 20 + r + 31, seed=200 + r + off)
            p, q = off + 20, off + 20 + r + 1
            s2 = s[:p] + other_base(s[p]) + s[p + 1:]
            out.append((f"sub_run{r}_at{off}", s, s2[:q] + other_base(s[q]) + s2[q + 1:]))
            out.append((f"ins_run{r}_at{off}", s, s2[:q] + other_base(s[q]) + s2[q:]))
            out.append((f"del_run{r}_at{off}", s, s2[:q] + s2[q + 1:]))
    # a run that ends exactly at the checkpoint column / at row 0: the edit sits r bases right of column 256 / of the start
    for r in RUN_N:
        for off in (0, 256):
            s = rand_seq(off + r + 40, seed=300 + r + off)
            q = off + r
            out.append((f"sub_after{r}_from{off}", s, s[:q] + other_base(s[q]) + s[q + 1:]))
    out.append(("homopolymer_290", b"A" * 300, b"A" * 290))
    out.append(("homopolymer_310", b"A" * 300, b"A" * 310))
    wide = rand_seq(300, seed=41)
    for rows in (3, 40, 41):
        tall = wide[130:130 + rows]
        out.append((f"clamp_{rows}rows", wide, tall))
        out.append((f"clamp_{rows}cols", tall, wide))
    return out


# the preset; no x-drop; odd and tiny max_g (midpoint early-out at level 1, and at "level 0" = never; two edits succeed AT max_g = 2)
EXT_KWS = [dt_kw(40, 10), dt_kw(40, 0), dt_kw(3, 1000), dt_kw(2, 10), dt_kw(1, 0), NO_DT]


# ---- (d) re-fill strips and the scratch limit ----
REFILL_M = [base + d for base in (2048, 4096, 6144, 8192) for d in (-64, -1, 0, 1, 64)]
REFILL_KWS = [NO_DT, dt_kw(40, 10)]


def _cgt(n: int, seed: int) -> bytes:
    return bytes(b"CGT"[x % 3] for x in rand_seq(n, seed=seed))


def refill_tail_pair(m: int):
    """700 common bases, then 40 columns of C against a run of A that brings b to m rows: the last block's re-fill doubles its height
    until it spans all of b."""
    y = _cgt(700, 51)
    return y + b"C" * 40, y + b"A" * (m - 700)


def refill_mid_pair(m: int):
    """The same run in the middle of the second block (column 300)."""
    y = _cgt(700, 51)
    return y, y[:300] + b"A" * (m - 700) + y[300:]


ORDINARY = gen_pair(500, 0.1, seed=2)  # rides along in every re-fill batch
