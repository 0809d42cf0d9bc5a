"""The gap-affine oracle of tests/affine_plain.py against answers found another way: closed forms, the unit-cost oracle, a textbook LCS,
and a second, deliberately naive cell-by-cell Gotoh that walks its value matrices with the reference's first-parent rule.  The GPU
tests (test_gpu_affine.py) rest on this oracle."""
import numpy as np
import pytest

import oracle
from astar_pairwise_aligner_amd import AffineCost
from tests import affine_plain as ap


def rand_seq(rng, n: int, alphabet: bytes = b"ACGT") -> bytes:
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


MODELS = {
    "lcs": AffineCost.lcs(),
    "unit": AffineCost.unit(),
    "linear": AffineCost.linear(3, 2),
    "linear_asymmetric": AffineCost.linear_asymmetric(2, 1, 3),
    "affine": AffineCost.affine(4, 6, 2),
    "linear_affine": AffineCost.linear_affine(3, 2, 4, 1),
    "affine_asymmetric": AffineCost.affine_asymmetric(5, 3, 1, 7, 2),
}


def naive(a: bytes, b: bytes, cm):
    cost, ops = naive_walk(a, b, cm)
    return cost, ap.cigar_text(ops)


def naive_ops(a: bytes, b: bytes, cm):
    return naive_walk(a, b, cm)[1]


def naive_walk(a: bytes, b: bytes, cm):
    """Cell by cell, with value matrices: AffineNwFront::first_col / next_front, then AffineNwFronts::trace with parent()."""
    n, m = len(a), len(b)
    sub, ins, dl, io, ie, do, de = ap.edge_costs(cm)
    INF = ap.INF
    M = [[INF] * (m + 1) for _ in range(n + 1)]
    Il = [[INF] * (m + 1) for _ in range(n + 1)]
    Dl = [[INF] * (m + 1) for _ in range(n + 1)]
    layers = {"M": M, "I": Il, "D": Dl}

    def parents(i, j, layer):  # iterate_parents: (di, dj, layer, cost, op)
        out = []
        if layer == "M":
            if i > 0 and j > 0 and a[i - 1] == b[j - 1]:
                out.append((-1, -1, "M", 0, "="))
            elif sub is not None:
                out.append((-1, -1, "M", sub, "X"))
            if ins is not None:
                out.append((0, -1, "M", ins, "I"))
            if dl is not None:
                out.append((-1, 0, "M", dl, "D"))
            if io is not None:
                out.append((0, 0, "I", ie, ""))
            if do is not None:
                out.append((0, 0, "D", de, ""))
        elif layer == "I":
            out += [(0, -1, "M", io, "i"), (0, -1, "I", ie, "i")]
        else:
            out += [(-1, 0, "M", do, "d"), (-1, 0, "D", de, "d")]
        return out

    def get(i, j, layer):
        return layers[layer][i][j] if i >= 0 and j >= 0 else None

    order = (["I"] if io is not None else []) + (["D"] if do is not None else []) + ["M"]
    for i in range(n + 1):
        for j in range(m + 1):
            for layer in order:
                if (i, j, layer) == (0, 0, "M"):
                    M[0][0] = 0
                    continue
                best = INF
                for di, dj, pl, c, _ in parents(i, j, layer):
                    v = get(i + di, j + dj, pl)
                    if v is not None:
                        best = min(best, v + c)
                layers[layer][i][j] = best
    ops = []
    st = (n, m, "M")
    while st != (0, 0, "M"):
        i, j, layer = st
        cur = layers[layer][i][j]
        for di, dj, pl, c, op in parents(i, j, layer):
            v = get(i + di, j + dj, pl)
            if v is not None and v + c == cur:
                st = (i + di, j + dj, pl)
                if op:
                    ops.append(op)
                break
        else:
            raise AssertionError("no parent")
    return M[n][m], ops[::-1]


def test_closed_forms():
    for name, cm in MODELS.items():
        for s in (b"", b"A", b"ACGTTGCA"):
            assert ap.affine_nw(s, s, cm) == (0, f"{len(s) if len(s) > 1 else ''}=" if s else ""), name
    cm = AffineCost.affine(4, 6, 2)
    for L in (1, 2, 5):
        x = b"ACGTACGT"
        y = x[:4] + b"G" * L + x[4:]
        c, g = ap.affine_nw(x, y, cm)
        assert c == 6 + 2 * L
        assert ap.affine_verify(g, x, y, cm) == c
        c, g = ap.affine_nw(y, x, cm)
        assert c == 6 + 2 * L and "D" in g and "I" not in g
    # empty sides: a gap of the whole other sequence
    assert ap.affine_nw(b"", b"ACGTA", cm) == (6 + 10, "5I")
    assert ap.affine_nw(b"ACG", b"", cm) == (6 + 6, "3D")
    assert ap.affine_nw(b"", b"ACGTA", AffineCost.linear(1, 3))[0] == 15
    assert ap.affine_nw(b"ACGTA", b"", AffineCost.linear_affine(1, 2, 4, 1))[0] == min(10, 4 + 5)
    # substitutions only
    assert ap.affine_nw(b"AAAA", b"ACCA", AffineCost.affine(4, 6, 2)) == (8, "=2X=")
    assert ap.affine_nw(b"AAAA", b"CCCC", AffineCost.linear(1, 5)) == (4, "4X")


def test_unit_equals_levenshtein():
    rng = np.random.default_rng(1)
    for _ in range(40):
        x = rand_seq(rng, int(rng.integers(0, 60)))
        y = rand_seq(rng, int(rng.integers(0, 60)))
        c, g = ap.affine_nw(x, y, AffineCost.unit())
        assert c == oracle.levenshtein(x, y)
        assert ap.affine_verify(g, x, y, AffineCost.unit()) == c


def _lcs(x, y):
    L = [[0] * (len(y) + 1) for _ in range(len(x) + 1)]
    for i in range(1, len(x) + 1):
        for j in range(1, len(y) + 1):
            L[i][j] = L[i - 1][j - 1] + 1 if x[i - 1] == y[j - 1] else max(L[i - 1][j], L[i][j - 1])
    return L[-1][-1]


def test_lcs_model_against_textbook_lcs():
    rng = np.random.default_rng(2)
    for _ in range(30):
        x = rand_seq(rng, int(rng.integers(0, 40)))
        y = rand_seq(rng, int(rng.integers(0, 40)))
        c, g = ap.affine_nw(x, y, AffineCost.lcs())
        assert c == len(x) + len(y) - 2 * _lcs(x, y)
        assert "X" not in g


@pytest.mark.parametrize("name", sorted(MODELS))
def test_against_naive_gotoh(name):
    cm = MODELS[name]
    rng = np.random.default_rng(hash(name) % 1000)
    for t in range(25):
        x = rand_seq(rng, int(rng.integers(0, 18)))
        y = rand_seq(rng, int(rng.integers(0, 18)))
        if t % 3 == 0:  # related pairs, so that long matches and gaps occur
            y = x[: len(x) // 2] + rand_seq(rng, int(rng.integers(0, 5))) + x[len(x) // 2 + int(rng.integers(0, 3)):]
        want = naive(x, y, cm)
        got = ap.affine_nw(x, y, cm)
        assert got == want, (x, y)
        assert ap.affine_verify(got[1], x, y, cm) == got[0]
        assert ap.no_adjacent_same_op(got[1])


def test_homopolymer_gap_position():
    # diagonal first in the main layer and open before extend in the affine layers: walking back, the matches at the end of the run
    # are taken first, so the gap lands at the start of the run
    cm = AffineCost.affine(4, 6, 2)
    assert naive(b"CAAAG", b"CAAAAAG", cm) == ap.affine_nw(b"CAAAG", b"CAAAAAG", cm) == (10, "=2I4=")
    assert naive(b"CAAAAAG", b"CAAAG", cm) == ap.affine_nw(b"CAAAAAG", b"CAAAG", cm) == (10, "=2D4=")
    cm = AffineCost.unit()
    assert ap.affine_nw(b"GAAT", b"GAAAT", cm) == naive(b"GAAT", b"GAAAT", cm) == (1, "=I3=")


def test_linear_vs_affine_tie():
    # linear_affine(sub, indel=2, open=2, extend=1): a gap of 2 costs 4 either way; the main layer offers the linear insertion before
    # the close of the insert layer, so the walk takes the linear edges (the naive walk records which: 'I' linear, 'i' affine)
    cm = AffineCost.linear_affine(10, 2, 2, 1)
    c, g = ap.affine_nw(b"ACGT", b"ACCCGT", cm)
    assert (c, g) == naive(b"ACGT", b"ACCCGT", cm) == (4, "=2I3=")
    assert naive_ops(b"ACGT", b"ACCCGT", cm) == list("=II===")
    assert ap.affine_verify(g, b"ACGT", b"ACCCGT", cm) == 4
    # a longer gap is cheaper affine (2 + L < 2 L for L > 2)
    c, g = ap.affine_nw(b"ACGT", b"ACCCCCGT", cm)
    assert (c, g) == naive(b"ACGT", b"ACCCCCGT", cm) == (6, "=4I3=")
    assert naive_ops(b"ACGT", b"ACCCCCGT", cm) == list("=iiii===")


def test_verify_rejects_bad_cigars():
    cm = AffineCost.affine(4, 6, 2)
    for bad in ("3=", "5=", "=X=", "2=I="):
        with pytest.raises(AssertionError):
            ap.affine_verify(bad, b"ACGT", b"ACGT", cm)
    assert ap.affine_verify("4=", b"ACGT", b"ACGT", cm) == 0


def test_any_byte_alphabet():
    cm = AffineCost.affine(4, 6, 2)
    x, y = bytes([0, 255, 7, 0, 65]), bytes([0, 255, 0, 65, 97])
    c, g = ap.affine_nw(x, y, cm)
    assert (c, g) == naive(x, y, cm)
    assert ap.affine_verify(g, x, y, cm) == c
