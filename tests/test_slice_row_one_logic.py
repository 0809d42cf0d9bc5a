"""The single row of the bit-sliced kernel (csrc/slice_kernel.hpp, PA_SLICE_ROW_ONE): the last row of a lane that owns an ODD number of rows.
Like the pair block it is inline asm, so this test reads the macro's asm text and interprets it on numpy uint32 words, with the
interpreter of tests/test_slice_row_logic.py:
  1. it is row A of PA_SLICE_ROW_PAIR, instruction for instruction (same opcodes, same immediates, same operand order);
  2. every valid cell -- eq in {0, 1}, dv and dh in {-1, 0, +1}: 18 cells -- against the cell rule d = min(1 - eq, dv + 1, dh + 1),
     dv' = d - dh, dh' = d - dv;
  3. a model of the kernel's skewed lanes with R = 3 and R = 5 rows per lane -- lane l works on column t - l at step t and takes the
     column's planes and the bottom row's (hp, hm) from the lane above a step later; (R - 1) / 2 pair blocks, then the single row; lanes
     in front of column 0 run on the neutral border (0, ~0) -- on random ragged groups of 32 pairs against a plain DP.
CPU only: no hipcc, no GPU."""
import re

import numpy as np
import pytest

from tests import strip_plain
from tests.test_slice_row_logic import KERNEL, ONES, _bits, _compile, _delta, _planes
from tests.test_slice_row_logic import _macro as _pair_macro


def _macro(name):
    """(instructions, {asm operand name: macro parameter or local}) of the macro `name`."""
    txt = KERNEL.read_text()
    defs = [m.start() for m in re.finditer(rf"^#define {name}\(", txt, re.M)]
    assert len(defs) == 1, f"{len(defs)} definitions of {name}"
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


ONE_PARAMS = ("vpA", "vmA", "nb0A", "nb1A", "a0", "a1", "hpp", "hmp", "hpo", "hmo")


@pytest.fixture(scope="module")
def row_one():
    ins, binds = _macro("PA_SLICE_ROW_ONE")
    for p in ONE_PARAMS:
        assert p in binds.values(), f"the asm does not bind {p}"
    return _compile(ins, binds)


@pytest.fixture(scope="module")
def row_pair():
    return _compile(*_pair_macro())


def test_is_row_a_of_the_pair_block():
    one, one_binds = _macro("PA_SLICE_ROW_ONE")
    pair, pair_binds = _pair_macro()
    assert len(one) == 7
    # row A's instructions of the pair block: those that write one of row A's registers (its z, hm, hp, vp, vm)
    row_a = [l for l in pair if re.match(r"v_\w+\s+%\[(zA|hmA|hpA|vpA_|vmA_)\]", l)]
    assert one == row_a
    # ... bound to the same things, except that the single row's (hp, hm) are the block's outputs
    want = {k: v for k, v in pair_binds.items() if re.search(r"%\[" + k + r"\]", " ".join(row_a))}
    want.update({"hmA": "hmo", "hpA": "hpo"})
    assert one_binds == want


def test_every_valid_cell(row_one):
    cases = np.array([(e, v, h) for e in (0, 1) for v in (-1, 0, 1) for h in (-1, 0, 1)])
    assert len(cases) == 18
    e, v, h = cases.T
    env = {"a0": np.zeros(18, np.uint32), "a1": np.zeros(18, np.uint32)}
    env["nb0A"], _ = _bits(e)  # eq = (a0 ^ nb0) & (a1 ^ nb1): with a = 0, a row matches where its negated code bits are both 1
    env["nb1A"] = env["nb0A"].copy()
    env["vpA"], env["vmA"] = _bits(v)
    env["hpp"], env["hmp"] = _bits(h)
    row_one(env)
    d = np.minimum(np.minimum(1 - e, v + 1), h + 1)
    assert np.array_equal(_delta(env["vpA"], env["vmA"]), d - h)
    assert np.array_equal(_delta(env["hpo"], env["hmo"]), d - v)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("R", [3, 5])
def test_skewed_lanes_with_odd_rows_against_plain_dp(row_pair, row_one, R, seed):
    rng = np.random.default_rng(100 * R + seed)
    G = 4  # groups stepped side by side: element g of every word is group g
    groups = []
    for _ in range(G):
        pairs = []
        for p in range(32):
            n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
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
    L = -(-max(len(b) for g in groups for _, b in g) // R)  # lanes; the rows past |b| are padding that nothing reads
    M = L * R
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
    zero = np.zeros(G, np.uint32)
    # the pipeline registers of every lane: the column's planes and the bottom row's (hp, hm) of the step before; (0, ~0) = neutral border
    pipe = [(zero, zero, zero, np.full(G, ONES)) for _ in range(L)]
    got = np.full((G, 32), -1, np.int64)
    for t in range(N + L - 1):
        before = list(pipe)
        for l in range(L):
            if l == 0:  # the chunk registers: column t (the pad behind the last column reads as zeros), the top row: +1 everywhere
                a0, a1 = (A0[t], A1[t]) if t < N else (zero, zero)
                hp, hm = np.full(G, ONES), zero
            else:
                a0, a1, hp, hm = before[l - 1]
            r0 = l * R
            for i in range(r0, r0 + R - 1, 2):
                env = {"vpA": vp[i], "vmA": vm[i], "vpB": vp[i + 1], "vmB": vm[i + 1], "nb0A": NB0[i], "nb1A": NB1[i], "nb0B": NB0[i + 1],
                       "nb1B": NB1[i + 1], "a0": a0, "a1": a1, "hpp": hp, "hmp": hm}
                row_pair(env)
                vp[i], vm[i], vp[i + 1], vm[i + 1] = env["vpA"], env["vmA"], env["vpB"], env["vmB"]
                hp, hm = env["hpo"], env["hmo"]
            i = r0 + R - 1
            env = {"vpA": vp[i], "vmA": vm[i], "nb0A": NB0[i], "nb1A": NB1[i], "a0": a0, "a1": a1, "hpp": hp, "hmp": hm}
            row_one(env)
            vp[i], vm[i] = env["vpA"], env["vmA"]
            pipe[l] = (a0, a1, env["hpo"], env["hmo"])
            done = t - l + 1  # columns this lane has finished: capture its rows of the pairs whose a ends here
            for g, pairs in enumerate(groups):
                for p, (a, b) in enumerate(pairs):
                    if len(a) == done:
                        bit = np.uint32(1 << p)
                        part = sum(int((vp[r][g] & bit) != 0) - int((vm[r][g] & bit) != 0) for r in range(r0, min(r0 + R, len(b))))
                        got[g, p] = part + (got[g, p] if got[g, p] >= 0 else len(a))
    for g, pairs in enumerate(groups):
        for p, (a, b) in enumerate(pairs):
            s, _, _, _ = strip_plain.rect_dp(a, b, np.ones(len(a)), np.ones(len(b)))
            assert got[g, p] == s + len(b), (g, p, len(a), len(b))
