"""The bit-sliced kernel's column ring (csrc/slice_kernel.hpp, "The column ring"): one entry (a0, a1, hp_in, hm_in) per column at index
column mod ring size, written once per chunk of 64 columns (lane j writes column 64 q + j at the chunk top), read once per step by every
lane for the column it works on in the NEXT step, and once more at the chunk top, behind the write, for the chunk's first step.

  1. A model of the indices alone -- lanes skewed one column per lane, the operations in the kernel's order -- says for which ring sizes
     every lane finds the entry of its own column (lane 0: the boundary half of its own column) at every (lane, step) with 0 <= c < n, and
     the zeroed entries in front of column 0 while c < 0.  The kernel's order needs 128 entries (64 fail); the same ring written a whole
     chunk AHEAD of its reads -- the order a ring of code planes alone could use, which the constant leaves room for -- needs 192 (128
     fail).  The kernel's constant passes both.
  2. The same order with real data: the kernel's own row asm (the interpreter of tests/test_slice_row_logic.py) stepped by a model of the
     skewed lanes that takes a0 / a1 and lane 0's row above from the ring, against a plain DP on ragged groups of 32 pairs.
CPU only: no hipcc, no GPU."""
import re

import numpy as np
import pytest

from tests.test_slice_neutral_border import FAR, NO_EVENT, _pair, _plain
from tests.test_slice_row_logic import KERNEL, ONES, _compile, _macro, _planes

COLUMNS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)


def _ring_entries():
    m = re.search(r"constexpr int kRingEntries = (\d+);", KERNEL.read_text())
    assert m, "kRingEntries not found in slice_kernel.hpp"
    return int(m.group(1))


def ring_violations(ring, n, ahead=0, L=64, reread=True):
    """The kernel's order of ring writes and reads on column numbers alone -> the (lane, step, column, found) where a lane did not get the
    entry of its column.  ahead = 1: the columns of chunk q + 1 are written at the top of chunk q instead (chunk 0's before the loop)."""
    slot = [None] * ring
    for j in range(L):
        slot[(ring - L + j) % ring] = ("front", j - L)  # zeroed once per job: what the lanes in front of column 0 read
    bad = []
    nchunks = (n + L - 1 + L - 1) // L
    if ahead:
        for j in range(L):
            slot[j % ring] = j
    held = [None] * L
    for q in range(nchunks):
        for j in range(L):  # the chunk top: lane j writes its column
            slot[(L * (q + ahead) + j) % ring] = L * (q + ahead) + j
        if (reread and not ahead) or q == 0:
            held = [slot[(L * q - l) % ring] for l in range(L)]  # ... and every lane reads the entry of the chunk's first step behind it
        for j in range(min(L, n + L - 1 - L * q)):
            t = L * q + j
            for l in range(L):
                c = t - l
                want = c if c >= 0 else ("front", c)
                if c < n and held[l] != want:
                    bad.append((l, t, c, held[l]))
            held = [slot[(t + 1 - l) % ring] for l in range(L)]  # behind the rows: the entry of the next step's column
    return bad


def test_the_constant():
    ring = _ring_entries()
    assert ring >= 192 and ring & (ring - 1) == 0, ring
    txt = KERNEL.read_text()
    assert "__shared__ uint4 ring[kRingEntries];" in txt
    assert "constexpr uint32_t kRingMask = (uint32_t)(kRingEntries - 1) * 16u;" in txt
    assert "ring[col & (kRingEntries - 1)] = make_uint4(cA.x, cA.y, cH.x, cH.y);" in txt, "the chunk's write"
    assert "ring[kRingEntries - 64 + lane] = make_uint4(0u, 0u, 0u, ~0u);" in txt, "the entries in front of column 0"
    assert "(uint32_t)(cnt16 - 16) & kRingMask" in txt and "(uint32_t)cnt16 & kRingMask" in txt, "the two reads"


@pytest.mark.parametrize("n", COLUMNS)
def test_ring_sizes(n):
    for ring in (128, 192, 256, _ring_entries()):
        assert not ring_violations(ring, n), f"ring of {ring}, the kernel's order"
    for ring in (192, 256, _ring_entries()):
        assert not ring_violations(ring, n, ahead=1), f"ring of {ring}, written a chunk ahead"
    # too small: the first write already lands on the entries in front of column 0, later ones on columns that lanes further down still want
    assert ring_violations(64, n)
    assert ring_violations(128, n, ahead=1)
    if n > 64:
        assert any(c >= 0 for _, _, c, _ in ring_violations(64, n)) and any(c >= 0 for _, _, c, _ in ring_violations(128, n, ahead=1))


def test_lane_0_reads_its_column_only_behind_the_write():
    """Without the read at the chunk top lane 0 would keep what the last step of the chunk before read: an entry nobody had written yet."""
    bad = ring_violations(_ring_entries(), 257, reread=False)
    assert [(l, t) for l, t, _, _ in bad] == [(0, 64), (0, 128), (0, 192), (0, 256)]


def ring_group(row_pair, pairs, L, R, ring):
    """tests/test_slice_neutral_border.py's skewed_group with the kernel's ring: chunks of L columns, a ring of `ring` entries
    (a0, a1, hp_in, hm_in), every lane's a0 / a1 and lane 0's row above from the entry the lane read a step ago.  -> the distances."""
    n = max(len(a) for a, _ in pairs)
    m = max(len(b) for _, b in pairs)
    strip = L * R
    nstrips = -(-m // strip)
    rows = nstrips * strip
    A0, A1 = _planes([a for a, _ in pairs], n)
    b0, b1 = _planes([b for _, b in pairs], rows)
    NB0, NB1 = ~b0, ~b1
    for p, (_, b) in enumerate(pairs):
        NB0[len(b):] &= ~np.uint32(1 << p)
        NB1[len(b):] &= ~np.uint32(1 << p)
    events = sorted({len(a) for a, _ in pairs})
    masks = [sum(1 << p for p, (a, _) in enumerate(pairs) if len(a) == col) for col in events]
    V = np.zeros((rows, 2), np.uint32)
    H = np.full((max(nstrips - 1, 1), n, 2), ONES)
    lane = np.arange(L)
    garbage = np.random.default_rng(ring).integers(0, 1 << 32, (ring, 4), dtype=np.uint64).astype(np.uint32)
    for s in range(nstrips):
        has_in, has_out = s > 0, s + 1 < nstrips
        row0 = s * strip + lane * R
        nb0 = [NB0[row0 + i] for i in range(R)]
        nb1 = [NB1[row0 + i] for i in range(R)]
        vp = [np.full(L, ONES) for _ in range(R)]
        vm = [np.zeros(L, np.uint32) for _ in range(R)]
        o_hp, o_hm = np.zeros(L, np.uint32), np.full(L, ONES)
        off = np.where((lane == L - 1) & has_out, (-lane * 8) & 0xFFFFFFFF, FAR).astype(np.int64)
        cnt = 1 - lane
        ev_i = np.zeros(L, np.int64)
        ev_col = np.full(L, events[0], np.int64)
        slot = garbage.copy()  # what the job before left behind
        slot[ring - L + lane] = (0, 0, 0, ONES)
        for q in range((n + L - 1 + L - 1) // L):
            col = q * L + lane
            cA = np.array([(A0[c], A1[c]) if c < n else (0, 0) for c in col], np.uint32)  # (behind the last column: the pad)
            if has_in:
                assert not any(c < n and (H[s - 1, c, 0] & H[s - 1, c, 1]) for c in col), "the strip above has not written this chunk"
                cH = np.array([H[s - 1, c] if c < n else (ONES, ONES) for c in col], np.uint32)
            else:
                cH = np.tile(np.array([ONES, 0], np.uint32), (L, 1))
            slot[col % ring] = np.concatenate([cA, cH], axis=1)
            r = slot[(cnt - 1) % ring]
            for j in range(min(L, n + L - 1 - L * q)):
                t = q * L + j
                a0, a1 = r[:, 0].copy(), r[:, 1].copy()
                hp = np.concatenate([[r[0, 2]], o_hp[:-1]]).astype(np.uint32)
                hm = np.concatenate([[r[0, 3]], o_hm[:-1]]).astype(np.uint32)
                front = cnt - 1 < 0
                assert np.all(a0[front] == 0) and np.all(a1[front] == 0), "a lane in front of column 0 read something that was not zeroed"
                for i in range(0, R, 2):
                    env = {"vpA": vp[i], "vmA": vm[i], "vpB": vp[i + 1], "vmB": vm[i + 1], "nb0A": nb0[i], "nb1A": nb1[i], "nb0B": nb0[i + 1],
                           "nb1B": nb1[i + 1], "a0": a0, "a1": a1, "hpp": hp, "hmp": hm}
                    row_pair(env)
                    vp[i], vm[i], vp[i + 1], vm[i + 1] = env["vpA"], env["vmA"], env["vpB"], env["vmB"]
                    hp, hm = env["hpo"], env["hmo"]
                o_hp, o_hm = hp, hm
                r = slot[cnt % ring]  # the entry of the next step's column, c + 1 = cnt
                for l in np.nonzero(off < n * 8)[0]:
                    assert l == L - 1 and has_out and off[l] // 8 == t - l and np.all(H[s, off[l] // 8] == ONES)
                    H[s, off[l] // 8] = (hp[l], hm[l])
                off = (off + 8) & 0xFFFFFFFF
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
        out.append(len(a) + int(np.count_nonzero(V[: len(b), 0] & bit)) - int(np.count_nonzero(V[: len(b), 1] & bit)))
    return out


@pytest.fixture(scope="module")
def row_pair():
    return _compile(*_macro())


# (lanes = columns per chunk, rows per lane, columns, rows): the ring has 4 chunks, as 256 entries are 4 chunks of 64.  Columns below, at and
# beyond one chunk, two chunks and the ring's wrap; one to three strips
SHAPES = [(4, 2, 1, 7), (4, 2, 4, 8), (4, 2, 5, 9), (4, 4, 17, 33), (4, 2, 33, 24), (8, 2, 31, 40), (8, 2, 65, 17), (3, 4, 13, 30)]


@pytest.mark.parametrize("L,R,n,m", SHAPES)
def test_ragged_groups_through_the_ring(row_pair, L, R, n, m):
    rng = np.random.default_rng(L * 1000 + R * 100 + n * 10 + m)
    lens = [(n, m), (1, m), (n, 1)] + [(int(rng.integers(1, n + 1)), int(rng.integers(1, m + 1))) for _ in range(29)]
    pairs = [_pair(rng, x, y) for x, y in lens]
    assert ring_group(row_pair, pairs, L, R, 4 * L) == [_plain(a, b) for a, b in pairs]
    if L == 4:  # (two chunks: the smallest ring that the kernel's order allows)
        assert ring_group(row_pair, pairs, L, R, 2 * L) == [_plain(a, b) for a, b in pairs]
