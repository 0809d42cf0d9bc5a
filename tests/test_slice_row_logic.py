"""The row logic of the bit-sliced kernel (csrc/slice_kernel.hpp, PA_SLICE_ROW_PAIR) is inline asm: the compiler checks neither the
`bitop3:` immediates nor the order of the operands.  This test reads the asm text of the macro, interprets its instructions on numpy
uint32 words (bit p = pair p of a group, as in the kernel) and checks
  1. every valid cell -- eq in {0, 1}, the left column's delta dv and the row above's delta dh in {-1, 0, +1} -- against the cell rule
     d = min(1 - eq, dv + 1, dh + 1) (d = D(i, j) - D(i - 1, j - 1)), dv' = d - dh, dh' = d - dv, for both rows of the block;
  2. random groups of 32 ragged pairs stepped row pair by row pair from fresh borders, as the kernel does, whose distances
     |a| + sum over the rows < |b| of (vp - vm) at column |a| must equal a plain DP (tests/strip_plain.py).
CPU only: no hipcc, no GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import strip_plain

ROOT = Path(__file__).resolve().parent.parent
KERNEL = ROOT / "astar-pairwise-aligner_amd" / "csrc" / "slice_kernel.hpp"
ONES = np.uint32(0xFFFFFFFF)


def _macro():
    """(instructions, {asm operand name: macro parameter or local}) of the PA_SLICE_ROW_PAIR that the kernel uses."""
    txt = KERNEL.read_text()
    defs = [m.start() for m in re.finditer(r"^#define PA_SLICE_ROW_PAIR\(", txt, re.M)]
    assert len(defs) == 1, f"{len(defs)} definitions of PA_SLICE_ROW_PAIR"
    body = txt[defs[0]: txt.index("while (0)", defs[0])]
    asm = body[body.index("asm volatile(") + len("asm volatile("):]
    strings, rest = [], asm
    while True:
        m = re.match(r'\s*\\?\s*"((?:[^"\\]|\\.)*)"', rest)
        if not m:
            break
        strings.append(m.group(1))
        rest = rest[m.end():]
    code = "".join(strings).replace("\\n", "\n").replace("\\t", "")
    ins = [l.strip() for l in code.split("\n") if l.strip()]
    binds = dict(re.findall(r'\[(\w+)\]\s*"[^"]*"\s*\((\w+)\)', rest))
    return ins, binds


def _compile(ins, binds):
    """A function env -> None that runs the asm on env[parameter] (numpy uint32 arrays); locals of the block live in env too."""
    ops = []
    for line in ins:
        m = re.fullmatch(r"(v_\w+)\s+(.*?)(?:\s+bitop3:(0x[0-9a-fA-F]+|\d+))?", line)
        assert m, line
        op, imm = m.group(1), m.group(3)
        regs = [binds[r] for r in re.findall(r"%\[(\w+)\]", m.group(2))]
        assert len(regs) == len(m.group(2).split(",")), f"an operand that is not a named register: {line}"
        if op == "v_bitop3_b32":
            assert imm is not None and len(regs) == 4, line
            ops.append(("bitop3", regs[0], regs[1:], int(imm, 0)))
        else:
            assert imm is None, line
            n = {"v_xor_b32": 2, "v_or_b32": 2, "v_and_b32": 2, "v_or3_b32": 3}.get(op)
            assert n is not None, f"no model of `{op}` in this test: {line}"
            assert len(regs) == n + 1, line
            ops.append((op, regs[0], regs[1:], None))

    def run(env):
        for op, d, s, imm in ops:
            x = [env[r] for r in s]
            if op == "v_xor_b32":
                env[d] = x[0] ^ x[1]
            elif op == "v_or_b32":
                env[d] = x[0] | x[1]
            elif op == "v_and_b32":
                env[d] = x[0] & x[1]
            elif op == "v_or3_b32":
                env[d] = x[0] | x[1] | x[2]
            else:  # truth table: bit (S0 * 4 + S1 * 2 + S2) of the immediate
                r = np.zeros_like(x[0])
                for k in range(8):
                    if (imm >> k) & 1:
                        t0 = x[0] if k & 4 else ~x[0]
                        t1 = x[1] if k & 2 else ~x[1]
                        t2 = x[2] if k & 1 else ~x[2]
                        r |= t0 & t1 & t2
                env[d] = r

    return run


@pytest.fixture(scope="module")
def row_pair():
    ins, binds = _macro()
    for p in ("vpA", "vmA", "vpB", "vmB", "nb0A", "nb1A", "nb0B", "nb1B", "a0", "a1", "hpp", "hmp", "hpo", "hmo"):
        assert p in binds.values(), f"the asm does not bind {p}"
    return _compile(ins, binds)


def _bits(d):
    """delta -1 / 0 / +1 -> (plus, minus) words"""
    d = np.asarray(d)
    return np.where(d > 0, ONES, np.uint32(0)), np.where(d < 0, ONES, np.uint32(0))


def _delta(p, m):
    assert not np.any(p & m), "a plus and a minus bit at once"
    return (p != 0).astype(np.int64) - (m != 0).astype(np.int64)


def test_every_valid_cell(row_pair):
    # row A: (eqA, dvA, dh of the row above); row B: (eqB, dvB) with row A's dh' coming in -- 18 x 6 cases, each row sees all 18 cells
    cases = np.array([(ea, va, h, eb, vb) for ea in (0, 1) for va in (-1, 0, 1) for h in (-1, 0, 1) for eb in (0, 1) for vb in (-1, 0, 1)])
    ea, va, h, eb, vb = cases.T
    env = {"a0": np.zeros(len(cases), np.uint32), "a1": np.zeros(len(cases), np.uint32)}
    # eq = (a0 ^ nb0) & (a1 ^ nb1): with a = 0, a row matches where its negated code bits are both 1
    env["nb0A"], _ = _bits(ea)
    env["nb1A"] = env["nb0A"].copy()
    env["nb0B"], _ = _bits(eb)
    env["nb1B"] = env["nb0B"].copy()
    env["vpA"], env["vmA"] = _bits(va)
    env["vpB"], env["vmB"] = _bits(vb)
    env["hpp"], env["hmp"] = _bits(h)
    row_pair(env)
    dA = np.minimum(np.minimum(1 - ea, va + 1), h + 1)
    hA = dA - va
    dB = np.minimum(np.minimum(1 - eb, vb + 1), hA + 1)
    assert np.array_equal(_delta(env["vpA"], env["vmA"]), dA - h)
    assert np.array_equal(_delta(env["vpB"], env["vmB"]), dB - hA)
    assert np.array_equal(_delta(env["hpo"], env["hmo"]), dB - vb)


def _planes(codes, length):
    """codes of up to 32 sequences (lists of 0..3) -> two uint32 planes per position (bit p = sequence p's code bit), and a mask of the
    sequences that reach each position"""
    c = np.zeros((32, length), np.int64)
    live = np.zeros((32, length), bool)
    for p, s in enumerate(codes):
        c[p, : len(s)] = s
        live[p, : len(s)] = True
    w = (np.uint64(1) << np.arange(32, dtype=np.uint64))[:, None]
    p0 = ((c & 1).astype(np.uint64) * w).sum(0).astype(np.uint32)
    p1 = ((c >> 1).astype(np.uint64) * w).sum(0).astype(np.uint32)
    return p0, p1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ragged_groups_against_plain_dp(row_pair, seed):
    rng = np.random.default_rng(seed)
    G = 4  # groups stepped side by side: element g of every word is group g
    groups = []
    for _ in range(G):
        pairs = []
        for p in range(32):
            n, m = int(rng.integers(1, 70)), int(rng.integers(1, 70))
            a = rng.integers(0, 4, n)
            if p % 3 == 0:  # near-equal pairs too: long diagonal runs
                b = a.copy()[:m]
                flip = rng.random(len(b)) < 0.1
                b[flip] = rng.integers(0, 4, int(flip.sum()))
            else:
                b = rng.integers(0, 4, m)
            pairs.append((a, b))
        groups.append(pairs)
    N = max(len(a) for g in groups for a, _ in g)
    M = max(len(b) for g in groups for _, b in g)
    M += M % 2  # rows in pairs; the rows past |b| are padding that nothing reads
    A0 = np.zeros((N, G), np.uint32)
    A1 = np.zeros((N, G), np.uint32)
    NB0 = np.zeros((M, G), np.uint32)
    NB1 = np.zeros((M, G), np.uint32)
    for g, pairs in enumerate(groups):
        A0[:, g], A1[:, g] = _planes([a for a, _ in pairs], N)
        b0, b1 = _planes([b for _, b in pairs], M)
        NB0[:, g], NB1[:, g] = ~b0, ~b1  # the negated planes of the profile
    vp = [np.full(G, ONES) for _ in range(M)]  # the left column: +1 everywhere
    vm = [np.zeros(G, np.uint32) for _ in range(M)]
    got = np.zeros((G, 32), np.int64)
    for c in range(N):
        hp, hm = np.full(G, ONES), np.zeros(G, np.uint32)  # the top row: +1 everywhere
        for i in range(0, M, 2):
            env = {"vpA": vp[i], "vmA": vm[i], "vpB": vp[i + 1], "vmB": vm[i + 1], "nb0A": NB0[i], "nb1A": NB1[i], "nb0B": NB0[i + 1],
                   "nb1B": NB1[i + 1], "a0": A0[c], "a1": A1[c], "hpp": hp, "hmp": hm}
            row_pair(env)
            vp[i], vm[i], vp[i + 1], vm[i + 1] = env["vpA"], env["vmA"], env["vpB"], env["vmB"]
            hp, hm = env["hpo"], env["hmo"]
        for g, pairs in enumerate(groups):  # capture the pairs whose a ends after this column
            for p, (a, b) in enumerate(pairs):
                if len(a) == c + 1:
                    bit = np.uint32(1 << p)
                    got[g, p] = len(a) + sum(int((vp[r][g] & bit) != 0) - int((vm[r][g] & bit) != 0) for r in range(len(b)))
    for g, pairs in enumerate(groups):
        for p, (a, b) in enumerate(pairs):
            s, _, _, _ = strip_plain.rect_dp(a, b, np.ones(len(a)), np.ones(len(b)))
            assert got[g, p] == s + len(b), (g, p, len(a), len(b))
