"""The tiled double-affine traceback as a scheme, on the CPU: tests/affine4_tiles_plain.py (checkpoint pass, tile fills from a store that
raises on any other read, a walk that carries its state) against the full-matrix oracle of tests/affine4_plain.py, cost and CIGAR, with
tiles of 8 x 8 so that pairs of a few dozen bytes cross many tile edges in every layer."""
import numpy as np
import pytest

from astar_pairwise_aligner_amd import AffineCost
from tests import affine4_plain as a4
from tests import affine4_tiles_plain as t4
from tests.affine_plain import cigar_elems

DOUBLE = AffineCost.double_affine(4, 6, 2, 24, 1)
ASYMMETRIC = AffineCost(5, None, None, [("ins", 3, 3), ("del", 7, 2), ("ins", 15, 1), ("del", 20, 1)])
LINEAR_EDGES = AffineCost(3, 5, 4, [("ins", 4, 2), ("del", 3, 2), ("ins", 12, 1), ("del", 14, 1)])
MODELS = {"double_affine": DOUBLE, "asymmetric": ASYMMETRIC, "linear_edges": LINEAR_EDGES}
TR = TC = 8


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def path_tiles(cigar, tile_rows, tile_cols):
    """The distinct tiles of a path, from its CIGAR alone, in the order the path enters them from (0, 0)."""
    i = j = 0
    out = [(0, 0)]
    for k, op in cigar_elems(cigar):
        for _ in range(k):
            i, j = i + (op != "I"), j + (op != "D")
            t = t4.tile_of(i, j, tile_rows, tile_cols)
            if out[-1] != t:
                assert t not in out
                out.append(t)
    return out


def check(x, y, cm, tile_rows=TR, tile_cols=TC):
    want = a4.affine4_nw(x, y, cm)
    cost, cigar, visited, st = t4.affine4_tiled(x, y, cm, tile_rows, tile_cols)
    assert (cost, cigar) == want, (len(x), len(y), tile_rows, tile_cols)
    # one fill per tile of the path, entered in walk order; the checkpoints are what the header's formula counts
    assert [t for t, _ in visited] == (path_tiles(want[1], tile_rows, tile_cols)[::-1] if x or y else [])
    n, m = len(x), len(y)
    assert len(st.rows) == (t4.row_tiles(m, tile_rows) - 1) * (n + 1)
    assert len(st.cols) == ((n - 1) // tile_cols if n else 0) * (m + 1)
    return want, visited


def runs_of(cigar, op):
    """[(first state, last state)] of every run of `op` in the path."""
    out, i, j = [], 0, 0
    for k, o in cigar_elems(cigar):
        di, dj = (k, k) if o in "=X" else (0, k) if o == "I" else (k, 0)
        if o == op:
            out.append(((i, j), (i + di, j + dj)))
        i, j = i + di, j + dj
    return out


@pytest.mark.parametrize("L", (12, 60))  # under DOUBLE a gap of 12 lies in layer 0 / 1 (30 < 36), a gap of 60 in layer 2 / 3 (84 < 126)
def test_insertion_run_open_at_row_edges(L):
    rng = np.random.default_rng(L)
    y = rand_seq(rng, 100)
    x, b = y, y[:40 - L // 2] + rand_seq(rng, L, b"NRYK") + y[40 - L // 2:]
    (cost, cigar), visited = check(x, b, DOUBLE)
    assert cost == (30 if L == 12 else 84)
    assert runs_of(cigar, "I") == [((40 - L // 2, 40 - L // 2), (40 - L // 2, 40 + L // 2))]  # one run, across row 40 = 5 x 8
    entries = [s for _, s in visited if s[2] != 0]
    assert entries and all(layer == (1 if L == 12 else 3) for _, _, layer in entries)  # tiles entered inside the open layer


@pytest.mark.parametrize("L", (12, 60))
def test_deletion_run_open_at_column_edges(L):
    rng = np.random.default_rng(100 + L)
    y = rand_seq(rng, 100)
    a = y[:40 - L // 2] + rand_seq(rng, L, b"NRYK") + y[40 - L // 2:]
    (cost, cigar), visited = check(a, y, DOUBLE)
    assert cost == (30 if L == 12 else 84)
    assert runs_of(cigar, "D") == [((40 - L // 2, 40 - L // 2), (40 + L // 2, 40 - L // 2))]
    entries = [s for _, s in visited if s[2] != 0]
    assert entries and all(layer == (2 if L == 12 else 4) for _, _, layer in entries)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_empty_sides_and_tile_sized_pairs(name):
    rng = np.random.default_rng(5)
    for n, m in ((0, 0), (0, 1), (1, 0), (0, 30), (30, 0), (1, 1), (7, 7), (8, 8), (9, 9), (16, 17), (17, 16), (8, 33), (33, 8)):
        y = rand_seq(rng, m)
        check((y + rand_seq(rng, n))[:n] if n % 2 else rand_seq(rng, n), y, MODELS[name])


@pytest.mark.parametrize("name", ("double_affine", "asymmetric"))
def test_seeded_small_pairs(name):
    rng = np.random.default_rng(len(name))
    for k in range(50):
        m = int(rng.integers(0, 45))
        y = rand_seq(rng, m)
        x = bytearray(y)
        for _ in range(int(rng.integers(0, 5))):  # a few substitutions and gaps of either piece's length
            at = int(rng.integers(0, len(x) + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0 and x:
                x[min(at, len(x) - 1)] = b"ACGT"[int(rng.integers(0, 4))]
            elif kind == 1:
                x[at:at] = rand_seq(rng, int(rng.choice((1, 3, 14, 25))))
            else:
                del x[at:at + int(rng.choice((1, 3, 14, 25)))]
        check(bytes(x), y, MODELS[name], *((TR, TC) if k % 3 else (4, 16) if k % 2 else (16, 5)))


def test_identical_sequences_cross_tile_corners():
    y = rand_seq(np.random.default_rng(3), 16)
    (cost, cigar), visited = check(y, y, DOUBLE)
    assert (cost, cigar) == (0, "16=") and [t for t, _ in visited] == [(1, 1), (0, 0)]


def test_the_store_raises_outside_the_checkpoints_and_the_tile():
    rng = np.random.default_rng(9)
    y = rand_seq(rng, 30)
    x = y[:10] + y[14:]
    _, st = t4.checkpoint_pass(x, y, DOUBLE, TR, TC)
    with pytest.raises(KeyError):
        st.row(0, len(x) + 1)
    with pytest.raises(KeyError):
        st.row(3, 0)  # the last row tile keeps no boundary row
    with pytest.raises(KeyError):
        st.col((len(x) - 1) // TC, 0)  # no checkpoint at or after column |a|
    t4.fill_tile(st, x, y, DOUBLE, TR, TC, len(x), len(y))
    st.code(len(x), len(y))
    with pytest.raises(KeyError):
        st.code(len(x) - TC, len(y))  # another column tile
    with pytest.raises(KeyError):
        st.code(len(x), 24)  # another row tile
