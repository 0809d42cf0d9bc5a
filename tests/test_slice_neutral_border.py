"""The bit-sliced kernel (csrc/slice_kernel.hpp) has no lane predicate in its step: a lane that has not reached column 0 runs its rows
like every other lane and is kept in the left column's state (vp = ~0, vm = 0) by what it takes in, the NEUTRAL border (hp, hm) = (0, ~0),
which it also hands on.  This test interprets the kernel's own row asm (the interpreter of tests/test_slice_row_logic.py) and checks
  1. the neutral border itself: from vp = ~0, vm = 0 and input (0, ~0), for random a0, a1 and row codes, both rows of a block keep their
     state and the block puts out (0, ~0);
  2. a model of the skewed lanes written from the kernel -- pipeline registers that start as (a0, a1, hp, hm) = (0, 0, 0, ~0), every lane
     stepping in every step, lane 0 taking the chunk value (the pad behind the last column), the boundary store through a running byte
     offset with a range check of n * 8 bytes, the capture through a running column counter and a "no more events" value -- against a
     plain DP (tests/strip_plain.py): a few lanes x a few row pairs, fewer and more columns than lanes, one to three strips, ragged |a|
     with an event at column 1.
CPU only: no hipcc, no GPU."""
import re

import numpy as np
import pytest

from tests import strip_plain
from tests.test_slice_row_logic import KERNEL, ONES, _compile, _macro, _planes

NO_EVENT = -(1 << 31)
FAR = 0x7FFFFFF0


@pytest.fixture(scope="module")
def row_pair():
    return _compile(*_macro())


def test_kernel_starts_from_the_neutral_border():
    """The model below is written from these lines of the kernel; if they change, so must the model."""
    txt = KERNEL.read_text()
    assert re.search(r"uint32_t a0 = 0, a1 = 0, o_hp = 0, o_hm = ~0u;", txt)
    assert re.search(r"uint32_t off = \(lane == 63 && has_out\) \? \(uint32_t\)\(-lane\) \* 8u : 0x7FFFFFF0u;", txt)
    assert re.search(r"int cnt = 1 - lane;", txt) and re.search(r"constexpr int kNoEvent = INT32_MIN;", txt)
    assert "(unsigned)c < (unsigned)n" not in txt, "the lane predicate is back"


def test_neutral_border_keeps_the_left_column(row_pair):
    rng = np.random.default_rng(5)
    k = 4096
    env = {name: rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32) for name in ("a0", "a1", "nb0A", "nb1A", "nb0B", "nb1B")}
    env.update(vpA=np.full(k, ONES), vmA=np.zeros(k, np.uint32), vpB=np.full(k, ONES), vmB=np.zeros(k, np.uint32),
               hpp=np.zeros(k, np.uint32), hmp=np.full(k, ONES))
    row_pair(env)
    for name in ("vpA", "vpB", "hmo"):
        assert np.all(env[name] == ONES), name
    for name in ("vmA", "vmB", "hpo"):
        assert np.all(env[name] == 0), name


def skewed_group(row_pair, pairs, L, R):
    """The kernel's schedule for one group of up to 32 pairs, with L lanes of R rows each (the kernel: 64 lanes): strips of L * R rows one
    after the other, each over steps 0 .. n + L - 2, lane l on column t - l at step t.  Words are numpy arrays over the lanes.
    -> the distance of every pair."""
    n = max(len(a) for a, _ in pairs)
    m = max(len(b) for _, b in pairs)
    strip = L * R
    nstrips = -(-m // strip)
    rows = nstrips * strip
    A0, A1 = _planes([a for a, _ in pairs], n)
    b0, b1 = _planes([b for _, b in pairs], rows)
    NB0, NB1 = ~b0, ~b1
    for p, (_, b) in enumerate(pairs):  # the rows past |b| of a pair are padding: zero words in the kernel's row planes
        NB0[len(b):] &= ~np.uint32(1 << p)
        NB1[len(b):] &= ~np.uint32(1 << p)
    events = sorted({len(a) for a, _ in pairs})
    masks = [sum(1 << p for p, (a, _) in enumerate(pairs) if len(a) == col) for col in events]
    V = np.zeros((rows, 2), np.uint32)
    H = np.full((max(nstrips - 1, 1), n, 2), ONES)  # boundary rows: "not written yet"
    lane = np.arange(L)
    for s in range(nstrips):
        has_in, has_out = s > 0, s + 1 < nstrips
        row0 = s * strip + lane * R
        nb0 = [NB0[row0 + i] for i in range(R)]
        nb1 = [NB1[row0 + i] for i in range(R)]
        vp = [np.full(L, ONES) for _ in range(R)]
        vm = [np.zeros(L, np.uint32) for _ in range(R)]
        a0, a1 = np.zeros(L, np.uint32), np.zeros(L, np.uint32)
        o_hp, o_hm = np.zeros(L, np.uint32), np.full(L, ONES)
        off = np.where((lane == L - 1) & has_out, (-lane * 8) & 0xFFFFFFFF, FAR).astype(np.int64)
        cnt = 1 - lane
        ev_i = np.zeros(L, np.int64)
        ev_col = np.full(L, events[0], np.int64)
        for t in range(n + L - 1):
            # lane 0: the chunk value -- behind the last column the pad (whatever it holds; here the planes' zero and an unwritten boundary)
            ca0, ca1 = (A0[t], A1[t]) if t < n else (np.uint32(0), np.uint32(0))
            if has_in and t < n:
                assert not (H[s - 1, t, 0] & H[s - 1, t, 1]), "the strip above has not written this column"
                chp, chm = H[s - 1, t]
            elif has_in:
                chp, chm = ONES, ONES
            else:
                chp, chm = ONES, np.uint32(0)
            a0 = np.concatenate([[ca0], a0[:-1]]).astype(np.uint32)
            a1 = np.concatenate([[ca1], a1[:-1]]).astype(np.uint32)
            hp = np.concatenate([[chp], o_hp[:-1]]).astype(np.uint32)
            hm = np.concatenate([[chm], o_hm[:-1]]).astype(np.uint32)
            for i in range(0, R, 2):
                env = {"vpA": vp[i], "vmA": vm[i], "vpB": vp[i + 1], "vmB": vm[i + 1], "nb0A": nb0[i], "nb1A": nb1[i], "nb0B": nb0[i + 1],
                       "nb1B": nb1[i + 1], "a0": a0, "a1": a1, "hpp": hp, "hmp": hm}
                row_pair(env)
                vp[i], vm[i], vp[i + 1], vm[i + 1] = env["vpA"], env["vmA"], env["vpB"], env["vmB"]
                hp, hm = env["hpo"], env["hmo"]
            o_hp, o_hm = hp, hm
            for l in np.nonzero(off < n * 8)[0]:  # the store: dropped outside the descriptor's n * 8 bytes
                assert l == L - 1 and has_out and off[l] % 8 == 0
                assert off[l] // 8 == t - l and np.all(H[s, off[l] // 8] == ONES), "one store per column, at the lane's column"
                H[s, off[l] // 8] = (hp[l], hm[l])
            off = (off + 8) & 0xFFFFFFFF  # (32 bits: lane L - 1's offset comes up to 0 from -8 (L - 1); the others must never get into range)
            assert not np.any(cnt == NO_EVENT)
            for l in np.nonzero(cnt == ev_col)[0]:
                assert cnt[l] == t - l + 1 and 1 <= cnt[l] <= n, "a capture outside the matrix"
                mask = np.uint32(masks[ev_i[l]])
                for i in range(R):
                    V[row0[l] + i] |= (vp[i][l] & mask, vm[i][l] & mask)
                ev_i[l] += 1
                ev_col[l] = events[ev_i[l]] if ev_i[l] < len(events) else NO_EVENT
            cnt = cnt + 1
        assert np.all(ev_col == NO_EVENT), "every lane has seen every event"
        if has_out:
            assert not np.any(H[s, :, 0] & H[s, :, 1]), "a boundary column was not written"
    out = []
    for p, (a, b) in enumerate(pairs):
        bit = np.uint32(1 << p)
        assert not np.any(V[:, 0] & V[:, 1] & bit)
        out.append(len(a) + int(np.count_nonzero(V[: len(b), 0] & bit)) - int(np.count_nonzero(V[: len(b), 1] & bit)))
    return out


def _pair(rng, n, m):
    a = rng.integers(0, 4, n)
    if rng.random() < 0.5:  # related: long diagonal runs
        b = np.resize(a, m).copy()
        flip = rng.random(m) < 0.15
        b[flip] = rng.integers(0, 4, int(flip.sum()))
    else:
        b = rng.integers(0, 4, m)
    return a, b


def _plain(a, b):
    s, _, _, _ = strip_plain.rect_dp(a, b, np.ones(len(a)), np.ones(len(b)))
    return s + len(b)


# (lanes, rows per lane, columns, rows): columns fewer than, equal to and more than the lanes; rows for one, two and three strips, ending on
# and one past a strip boundary
SHAPES = [(4, 2, 1, 1), (4, 2, 2, 8), (4, 4, 3, 17), (4, 4, 4, 33), (4, 4, 5, 16), (5, 2, 13, 21), (8, 2, 3, 40), (8, 4, 9, 33), (3, 6, 20, 37),
          (6, 2, 6, 12)]


@pytest.mark.parametrize("L,R,n,m", SHAPES)
def test_skewed_lanes_without_predicate(row_pair, L, R, n, m):
    rng = np.random.default_rng(L * 1000 + R * 100 + n * 10 + m)
    # ragged: the first pair is the widest and the tallest, one pair ends after column 1 (an event at column 1), one is one row tall
    lens = [(n, m), (1, m), (n, 1)] + [(int(rng.integers(1, n + 1)), int(rng.integers(1, m + 1))) for _ in range(29)]
    pairs = [_pair(rng, x, y) for x, y in lens]
    got = skewed_group(row_pair, pairs, L, R)
    assert got == [_plain(a, b) for a, b in pairs]


def test_skewed_lanes_equal_lengths(row_pair):
    """One event only, at the last column; fewer than 32 pairs."""
    rng = np.random.default_rng(3)
    pairs = [_pair(rng, 7, 19) for _ in range(5)]
    assert skewed_group(row_pair, pairs, 4, 4) == [_plain(a, b) for a, b in pairs]
