"""The plain DP of tests/search_plain.py against the reference's two documented search answers and against the CPU
oracle, so that the GPU edge tests (test_gpu_search_edges.py) rest on a reference that was checked on its own."""
import numpy as np
import pytest

from tests import search_plain as sp
from tests.util_seq import rand_seq

UCS = [0.0, 1.0, 0.5, 0.25, 0.3, 1 / 3, 0.1, 0.01, 0.999, 1e-6, 0.7]
PATTERN_LETTERS = b"ACGTNYR*acgtnyr"


def _pattern(rng, plen: int) -> bytes:
    return bytes(PATTERN_LETTERS[i] for i in rng.integers(0, len(PATTERN_LETTERS), plen))


def test_known_answers():
    assert sp.search(b"AC", b"CTTACTTA", 0.0) == [0, 0, 1, 2, 1, 0, 1, 2, 1, 0, 0]
    assert sp.search(b"CT", b"ACTG", 1.0) == [2, 2, 1, 0, 1, 2, 2]


def test_unmatched_prefix_is_float32():
    # 21 / 0.7 is 30.000000000000004 in double precision but exactly 30 in float32 (0.7f = 0.699999988): the marked row is
    # 30, not 31.  Rows 0, 2, 3, 5, 6, 8, ... come from ceil(i / 0.7) for i = 0, 1, 2, ...
    marked = lambda U: [r for r in range(len(U) - 1) if U[r + 1] > U[r]]  # noqa: E731
    m = marked(sp.unmatched_prefix(40, 0.7))
    assert 30 in m and 31 not in m
    assert m[:8] == [0, 2, 3, 5, 6, 8, 9, 10]
    assert marked(sp.unmatched_prefix(25, 0.3)) == [0, 4, 7, 10, 14, 17, 20, 24]
    assert sp.unmatched_prefix(10, 0.0).tolist() == [0] * 11
    assert sp.unmatched_prefix(5, 1.0).tolist() == [0, 1, 2, 3, 4, 5]
    assert sp.unmatched_prefix(4, 0.5).tolist() == [0, 1, 1, 2, 2]  # rows 0 and 2
    assert sp.unmatched_prefix(3, 1e-6).tolist() == [0, 1, 1, 1]  # row 0 only
    assert sp.unmatched_prefix(0, 0.5).tolist() == [0]


def test_float32_rows_against_oracle(oracle):
    """uc = 0.7 marks row 30 where a double-precision reading would mark row 31: the outputs differ at plen > 30."""
    pattern, text = b"A" * 40, b"C" * 50
    got = sp.search(pattern, text, 0.7)
    assert got == oracle.search(pattern, text, 0.7)
    assert got[0] == 28  # 28 of the forty rows are marked


def test_rejects_unknown_letters():
    with pytest.raises(ValueError):
        sp.search(b"ACX", b"ACGT", 0.0)
    with pytest.raises(ValueError):
        sp.search(b"AC", b"ACGN", 0.0)


def test_matches_oracle_random(oracle):
    rng = np.random.default_rng(2024)
    for case in range(300):
        plen = int(rng.integers(0, 301))
        tlen = int(rng.integers(0, 2001)) if case % 4 else int(rng.integers(0, 80))
        text = rand_seq(tlen, seed=int(rng.integers(1 << 30)))
        if case % 2:
            text = text.lower()
        elif case % 3 == 0 and tlen:  # mixed case
            text = bytes(c | (0x20 if k % 3 == 0 else 0) for k, c in enumerate(text))
        pattern = _pattern(rng, plen)
        if case % 5 == 0 and tlen > plen:  # a planted copy: low costs and real hits
            at = int(rng.integers(0, tlen - plen + 1))
            text = text[:at] + bytes(b"ACGT"[k % 4] if c in b"NnYyRr*" else c for k, c in enumerate(pattern.upper())) + text[at + plen:]
            if case % 2:
                text = text.lower()
        uc = UCS[case % len(UCS)]
        assert sp.search(pattern, text, uc) == oracle.search(pattern, text, uc), (case, plen, tlen, uc)


def test_matches_oracle_text_shorter_than_padding(oracle):
    """plen = 65 pads to 128 rows (padding 63): with tlen < 63 the dropped readout values reach into the right column."""
    rng = np.random.default_rng(7)
    for plen in (65, 100, 127):
        pattern = _pattern(rng, plen)
        for tlen in range(0, 128 - plen + 2):
            text = rand_seq(tlen, seed=1000 + tlen)
            uc = UCS[tlen % len(UCS)]
            assert sp.search(pattern, text, uc) == oracle.search(pattern, text, uc), (plen, tlen, uc)


def test_check_trace_accepts_oracle_traces(oracle):
    rng = np.random.default_rng(5)
    cases = [(b"AC", b"CTTACTTA", 0.0), (b"CT", b"ACTG", 1.0)]
    for k in range(40):
        plen = int(rng.integers(1, 40))
        tlen = int(rng.integers(0, 90))
        cases.append((_pattern(rng, plen), rand_seq(tlen, seed=k).lower() if k % 2 else rand_seq(tlen, seed=k), UCS[k % len(UCS)]))
    for pattern, text, uc in cases:
        out = sp.search(pattern, text, uc)
        for idx in range(len(out)):
            cigar, path = oracle.search_trace(pattern, text, uc, idx)
            sp.check_trace(pattern, text, uc, idx, out, cigar, path)


def test_check_trace_rejects_wrong_alignments(oracle):
    pattern, text, uc = b"ACGTACGT", b"TTTACGAACGTTT", 0.5
    out = sp.search(pattern, text, uc)
    idx = 11
    cigar, path = oracle.search_trace(pattern, text, uc, idx)
    sp.check_trace(pattern, text, uc, idx, out, cigar, path)
    bad = [
        (cigar, path, [v + 1 if k == idx else v for k, v in enumerate(out)]),  # cost does not add up
        (cigar, path[1:], out),  # path shorter than the CIGAR
        (cigar.replace("X", "="), path, out),  # a mismatch spelled as a match
        (cigar, [(i + 1, j) for i, j in path], out),  # ends elsewhere
    ]
    for c, p, o in bad:
        with pytest.raises(AssertionError):
            sp.check_trace(pattern, text, uc, idx, o, c, p)


def test_empty_pattern_trace_oracle(oracle):
    """search.rs:132-228 with an empty pattern: width 0, cost 0 = target, no step -- an empty CIGAR at (idx, 0)."""
    text = b"ACGTTGCA"
    out = sp.search(b"", text, 0.5)
    assert out == [0] * (len(text) + 1) == oracle.search(b"", text, 0.5)
    for idx in range(len(text) + 1):
        assert oracle.search_trace(b"", text, 0.5, idx) == ("", [(idx, 0)])
        sp.check_trace(b"", text, 0.5, idx, out, "", [(idx, 0)])
    assert oracle.search_trace(b"", b"", 0.0, 0) == ("", [(0, 0)])
    with pytest.raises(ValueError):
        oracle.search_trace(b"", text, 0.5, len(text) + 1)
