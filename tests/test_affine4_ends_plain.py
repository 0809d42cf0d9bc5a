"""The oracle of the double-affine ends-free tests (tests/affine4_ends_plain.py) against brute force: the cost is the least
general-gap cost of (a[s:e], b) over the allowed s <= e, by a DP that has no layers; `end` is the lowest minimiser of the last row; and
the CIGAR, priced on its own over a[start:end], costs just that."""
import numpy as np
import pytest

from tests.affine4_ends_cases import MODELS, SETTINGS
from tests.affine4_ends_plain import affine4_ends
from tests.affine4_plain import affine4_nw, affine4_verify, general_gap_cost


def small_pairs(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n, m = int(rng.integers(0, 14)), int(rng.integers(0, 10))
        out.append((bytes(b"AC"[k] for k in rng.integers(0, 2, n)), bytes(b"AC"[k] for k in rng.integers(0, 2, m))))
    return out + [(b"", b""), (b"ACCA", b""), (b"", b"CA")]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_oracle_against_brute_force(name):
    cm = MODELS[name]
    for a, b in small_pairs(len(name), 40):
        n = len(a)
        glob = {(s, e): general_gap_cost(a[s:e], b, cm) for s in range(n + 1) for e in range(s, n + 1)}
        for fs, fe in SETTINGS:
            cost, start, end, cigar, row = affine4_ends(a, b, cm, fs, fe)
            allowed = [(s, e) for s, e in glob if (fs or s == 0) and (fe or e == n)]
            assert cost == min(glob[se] for se in allowed), (a, b, fs, fe)
            # the last row: the best start for every end, and `end` its lowest minimiser
            assert row.tolist() == [min(glob[s, e] for s in range(e + 1) if fs or s == 0) for e in range(n + 1)]
            assert end == (int(np.argmin(row)) if fe else n) and row[end] == cost
            assert (fs or start == 0) and 0 <= start <= end
            assert affine4_verify(cigar, a[start:end], b, cm) == cost
            untraced = affine4_ends(a, b, cm, fs, fe, trace=False)
            assert (untraced[0], untraced[2]) == (cost, end)
        c, g = affine4_nw(a, b, cm)
        assert affine4_ends(a, b, cm)[:4] == (c, 0, n, g)  # both switches off: affine4_nw
