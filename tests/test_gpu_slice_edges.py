"""The bit-sliced full-DP kernel (csrc/slice_kernel.hpp, planned and launched by csrc/slice_unit.hip) at its structural edges and size limits.

test_gpu_slice.py draws its lengths at random; this file aims at the places where the kernel's layout changes:
  * columns: chunks of 64 (the last chunk's step count, the prefetch clamped into the pad), 32 columns per transpose wavefront, 128 per
    transpose block, 16 per code word;
  * rows: strips of 64 R rows, profile words of 64, score spans of 4096;
  * groups: sorting by (|a|, |b|, index), groups of 32 and the group of one at the end, capture events (one, 32, 50 k columns apart);
  * sizes: gridDim.y of the two transposes at and past 65 535 blocks, the admission bound of choose_rows_per_lane (2^27), pair counts
    past one encode launch (32 768 pairs).

Every distance is checked against oracle.levenshtein (a plain O(n m) DP, oracle/pa_oracle.c) or, past about 1e9 cells, against a closed
form that is exact: a substring of the other sequence costs the length difference, two one-letter sequences of different letters cost the
longer length, identity costs 0.  The pairs of a batch are chosen so that their distances are pairwise distinct (asserted), and every batch
is presented in reversed and in shuffled order, so a cost written to the wrong pair fails.  Every batch runs twice on the resident plan.
Batch.shape() is checked against a model of the plan written from slice_plan.hpp / slice_kernel.hpp (plan_model below)."""
import random
import time

import numpy as np
import pytest

from tests.util_seq import gen_pair, mutate, rand_seq

pytestmark = pytest.mark.gpu

SETTINGS = (28, 52, 1)  # PA_SLICE: the smallest and the largest instantiation (slice_plan.hpp kRowsPerLane), 1 = the library's own choice
SCORE_SPAN = 4096  # rows per wavefront of slice_score_kernel (kScoreSpan)
PAD = 64  # columns of pad on each side of a group's column planes (kPad)

# chunk (64), transpose wavefront (32 columns), transpose block (128 columns) and code word (16) boundaries.  A group runs n + 63 steps in
# chunks of 64: the last chunk has 1 step at n = 2, 66, 130 (n = 2 mod 64) and all 64 at n = 1, 65, 129, 193, 4097 (n = 1 mod 64); every n
# other than 0 or 1 mod 64 has the second-to-last chunk prefetch past column n + 63 (the clamp of pcol into the pad).
COLS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193, 4095, 4096, 4097)


def rows_edges(R):
    """|b| at the boundaries of profile words, strips of 64 R rows and score spans."""
    s = 64 * R
    return (1, 31, 32, 33, 63, 64, 65, s - 1, s, s + 1, 2 * s, 2 * s + 1, 4095, 4096, 4097, 8191, 8193)


ROWS = tuple(sorted(set(rows_edges(28)) | set(rows_edges(52))))  # 22 lengths; 8193 = three score spans, 5 strips at R = 28, 3 at R = 52


@pytest.fixture(scope="module")
def pa():
    import astar_pairwise_aligner_amd as pa

    pa.require_gpu()
    return pa


# ---- the plan, restated ------------------------------------------------------------------------------------------------------------------


def plan_model(lens, R):
    """What slice::create must plan for pairs of lengths `lens` at R rows per lane: live pairs (both sides non-empty) sorted by
    (|a|, |b|, index) in groups of 32; a group is as wide as its longest a (n) and has S = ceil(max |b| / 64 R) strips of 64 R rows; every
    group keeps n + 2 pad columns of planes, S * 64 R rows of row planes and as many captured rows, and S - 1 boundary rows of n + 2 pad."""
    live = sorted((n, m, i) for i, (n, m) in enumerate(lens) if n > 0 and m > 0)
    strip = 64 * R
    groups = jobs = cells = cols = rows = bounds = 0
    for g in range(0, len(live), 32):
        grp = live[g : g + 32]
        n, m = max(x[0] for x in grp), max(x[1] for x in grp)
        S = -(-m // strip)
        groups += 1
        jobs += S
        cells += S * strip * n * 32
        cols += n + 2 * PAD
        rows += S * strip
        bounds += (S - 1) * (n + 2 * PAD)
    return {"groups": groups, "jobs": jobs, "computed_cells": cells, "boundary_bytes": 8 * bounds, "device_bytes": 8 * (cols + 2 * rows + bounds)}


def test_plan_model_by_hand():
    """The model itself on two batches worked out by hand (needs no GPU itself)."""
    # 33 live pairs: the 32 shortest by (|a|, |b|, index) make group 0, the longest a is a group of one
    lens = [(10, 100)] * 20 + [(10, 5)] * 12 + [(0, 7), (7, 0)] + [(11, 1)]
    assert plan_model(lens, 28) == {"groups": 2, "jobs": 2, "computed_cells": 1792 * 10 * 32 + 1792 * 11 * 32, "boundary_bytes": 0,
                                    "device_bytes": 8 * ((138 + 139) + 2 * (1792 + 1792))}
    # one group, |b| = 2 * 64 * 52 + 1: three strips, two boundary rows of n + 128
    lens = [(300, 6657), (5, 1)]
    assert plan_model(lens, 52) == {"groups": 1, "jobs": 3, "computed_cells": 3 * 3328 * 300 * 32, "boundary_bytes": 8 * 2 * 428,
                                    "device_bytes": 8 * (428 + 2 * 3 * 3328 + 2 * 428)}


# ---- pairs with known distances ----------------------------------------------------------------------------------------------------------


def _fit(s, m, seed):
    return s[:m] if len(s) >= m else s + rand_seq(m - len(s), seed, 5)


def make_pair(kind, n, m, seed, oracle):
    """-> (a, b, distance) with |a| = n, |b| = m.  Closed forms where they are exact, oracle.levenshtein otherwise."""
    rng = random.Random(seed)
    if kind == "rand":  # unrelated
        a, b = rand_seq(n, seed, 1), rand_seq(m, seed, 2)
    elif kind == "mut":  # related, mixed divergence
        a = rand_seq(n, seed, 1)
        b = _fit(mutate(a, rng.choice([0.02, 0.1, 0.3]), seed), m, seed)
    elif kind in ("prefix", "suffix", "sub"):  # the shorter one is a prefix / suffix / interior substring of the longer one
        lo, hi = min(n, m), max(n, m)
        long_ = rand_seq(hi, seed, 3)
        off = {"prefix": 0, "suffix": hi - lo, "sub": rng.randint(1, hi - lo - 1) if hi - lo >= 2 else 0}[kind]
        short = long_[off : off + lo]
        a, b = (long_, short) if n >= m else (short, long_)
        return a, b, hi - lo
    elif kind.startswith("homo"):  # homoXY: X * n against Y * m
        x, y = (kind[4], kind[5]) if len(kind) == 6 else (rng.choice("ACGT"), rng.choice("ACGT"))
        return x.encode() * n, y.encode() * m, abs(n - m) if x == y else max(n, m)
    else:
        raise ValueError(kind)
    return a, b, oracle.levenshtein(a, b)


KINDS = ("rand", "mut", "prefix", "suffix", "sub", "homo")


def distinct_pairs(specs, oracle, seed, kinds=KINDS, dups=0, avoid=()):
    """specs: one (n choices, m choices) per pair.  Draws length, content kind and seed until the pair's distance differs from those of
    every pair drawn before it (and from `avoid`).  Then `dups` more pairs with the (|a|, |b|) of a pair already drawn and other contents
    (the sort's tie-break by index).  -> (pairs, distances)."""
    rng = random.Random(seed)
    pairs, want, used = [], [], set(avoid)

    def draw(ns, ms):
        for _ in range(400):
            n, m = ns() if callable(ns) else (rng.choice(ns), rng.choice(ms))
            a, b, d = make_pair(rng.choice(kinds), n, m, rng.randrange(1 << 40), oracle)
            if d not in used:
                used.add(d)
                pairs.append((a, b))
                want.append(d)
                return
        raise AssertionError(f"no pair with a new distance for {ns} x {ms}")

    for ns, ms in specs:
        draw(ns, ms)
    drawn = [(len(a), len(b)) for a, b in pairs]
    for _ in range(dups):
        draw(lambda: rng.choice(drawn), None)
    return pairs, want


def big_seq(n, seed):
    """n uniform bases (uint8 draws: a few hundred MB at most for the size-limit cases)."""
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)].tobytes()


# ---- running ---------------------------------------------------------------------------------------------------------------------------


def assert_plan(sh, lens, R):
    model = plan_model(lens, R)
    got = {"groups": sh["groups"], "jobs": sh["jobs"], "computed_cells": int(sh["computed_cells"]), "boundary_bytes": int(sh["boundary_bytes"]),
           "device_bytes": int(sh["device_bytes"])}
    assert got == model, (got, model)


def assert_costs(costs, pairs, want):
    bad = [i for i, (c, w) in enumerate(zip(costs.tolist(), want)) if c != w]
    assert not bad, f"{len(bad)} of {len(want)} wrong: " + ", ".join(f"#{i} |a|={len(pairs[i][0])} |b|={len(pairs[i][1])}: {int(costs[i])} != {want[i]}"
                                                                for i in bad[:8])


def run_sliced(pa, monkeypatch, setting, pairs, want, orders=("reversed", "shuffled"), distinct=True):
    """PA_SLICE=<setting>; the batch in each of `orders`: sliced (the forced R), the plan as modelled, the oracle's distances, twice."""
    if distinct:
        live = [w for (a, b), w in zip(pairs, want) if a and b]
        assert len(set(live)) == len(live), "the test's own pairs must have pairwise distinct distances"
    monkeypatch.setenv("PA_SLICE", str(setting))
    for order in orders:
        perm = list(range(len(pairs)))
        if order == "reversed":
            perm.reverse()
        elif order == "shuffled":
            random.Random(len(pairs) * 7 + setting).shuffle(perm)
        ps, ws = [pairs[i] for i in perm], [want[i] for i in perm]
        bt = pa.Batch(ps)
        try:
            sh = bt.shape()
            assert sh["kernel"].startswith("pa::slice::slice_kernel<"), sh
            if setting > 1:
                assert sh["sliced_rows_per_lane"] == setting, sh
            assert_plan(sh, [(len(a), len(b)) for a, b in ps], sh["sliced_rows_per_lane"])
            c1, _ = bt.run()
            c2, _ = bt.run()  # the resident plan again: V and the boundary rows are reset before every pass
        finally:
            bt.close()
        assert_costs(c1, ps, ws)
        assert np.array_equal(c1, c2)


# ---- b. column edges -----------------------------------------------------------------------------------------------------------------


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def column_group(n_max, oracle):
    """One group: |a| from the edges up to n_max (n_max itself once, so that it is the group's width), |b| up to 200, 4 duplicates of a
    pair's (|a|, |b|)."""
    below = [c for c in COLS if c < n_max]
    a_lens = [n_max] + [below[i % len(below)] for i in range(27)] if below else [n_max] * 28
    return distinct_pairs([((n,), tuple(range(1, 201))) for n in a_lens], oracle, seed=n_max, dups=4)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("n_max", COLS)
def test_column_edges(pa, oracle, monkeypatch, setting, n_max):
    pairs, want = cached(("cols", n_max), lambda: column_group(n_max, oracle))
    assert max(len(a) for a, _ in pairs) == n_max and len(pairs) == 32
    run_sliced(pa, monkeypatch, setting, pairs, want)


# ---- c. row edges --------------------------------------------------------------------------------------------------------------------


def row_group(oracle):
    """One group with every |b| of ROWS: the tallest (8193) crosses two score-span boundaries and runs 3 (R = 52) or 5 (R = 28) strips; the
    group also has pairs whose b ends in span 0 and pairs whose b ends exactly on a strip boundary (64 R, 128 R).  10 duplicates."""
    a_choices = (1, 2, 63, 64, 65, 127, 128, 129, 200, 333)
    return distinct_pairs([(a_choices, (m,)) for m in ROWS], oracle, seed=44, dups=32 - len(ROWS))


@pytest.mark.parametrize("setting", SETTINGS)
def test_row_edges(pa, oracle, monkeypatch, setting):
    pairs, want = cached("rows", lambda: row_group(oracle))
    tallest = max(len(b) for _, b in pairs)
    assert tallest > 2 * SCORE_SPAN and any(len(b) < SCORE_SPAN for _, b in pairs)
    if setting > 1:
        assert -(-tallest // (64 * setting)) >= 3 and any(len(b) % (64 * setting) == 0 for _, b in pairs)
    run_sliced(pa, monkeypatch, setting, pairs, want)


# ---- d. group composition and capture events -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("live", [1, 31, 32, 33, 65])
def test_group_counts(pa, oracle, monkeypatch, setting, live):
    """Groups that are not full; 33 and 65: the longest pair alone in the last group.  Two pairs with an empty side ride along."""
    def make():
        dups = min(3, live - 1)
        pairs, want = distinct_pairs([(tuple(range(1, 701)), tuple(range(1, 701)))] * (live - dups), oracle, seed=live, dups=dups)
        return pairs + [(b"", b"ACGTA"), (b"TTG", b"")], want + [5, 3]

    pairs, want = cached(("count", live), make)
    run_sliced(pa, monkeypatch, setting, pairs, want)


def one_event_group(oracle):
    """32 pairs with |a| = 1000: one capture event; the b are substrings of a (or a of b) of distinct lengths."""
    rng = random.Random(9)
    ms = rng.sample(range(1, 1000), 20) + rng.sample(range(1001, 2000), 12)
    return distinct_pairs([((1000,), (m,)) for m in ms], oracle, seed=9, kinds=("prefix", "suffix", "sub"))


def consecutive_group(oracle):
    """|a| = 50 .. 81: 32 capture events, one per column, across the chunk boundary at 64; the longest (81) is unique, at bit 31."""
    rng = random.Random(10)
    return distinct_pairs([((n,), tuple(range(1, 300))) for n in rng.sample(range(50, 82), 32)], oracle, seed=10)


def wide_group(oracle):
    """The shortest a is 1, the longest 50 000 (unique: bit 31): events at column 1 and 50 k columns later.  The pair with the smallest
    |a| has the largest |b| (captured first, the tallest)."""
    rng = random.Random(11)
    specs = [((1,), (6000,)), ((1,), (1, 2, 3, 4, 5, 6, 7, 8)), ((2,), (64, 65, 200))]
    specs += [((n,), tuple(range(1, 1500))) for n in (3, 17, 63, 64, 65, 128, 129, 500, 1000, 1024, 2047, 4096, 4097, 10_000, 20_000)]
    specs += [((rng.randint(3, 30_000),), tuple(range(1, 1500))) for _ in range(13)]
    specs += [((50_000,), tuple(range(64, 1500)))]
    return distinct_pairs(specs, oracle, seed=11)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("which", ["one_event", "consecutive", "wide"])
def test_capture_events(pa, oracle, monkeypatch, setting, which):
    make = {"one_event": one_event_group, "consecutive": consecutive_group, "wide": wide_group}[which]
    pairs, want = cached(which, lambda: make(oracle))
    assert len(pairs) == 32
    if which != "one_event":
        longest = max(len(a) for a, _ in pairs)
        assert sum(len(a) == longest for a, _ in pairs) == 1  # sorted last: bit 31
    if which == "wide":
        assert min(len(a) for a, _ in pairs) == 1 and max(len(a) for a, _ in pairs) >= 50_000
        assert len(pairs[0][1]) == max(len(b) for _, b in pairs)
    run_sliced(pa, monkeypatch, setting, pairs, want)


def test_no_live_pair(pa, monkeypatch):
    """>= 64 pairs, every one with an empty side: a sliced plan without groups (slice::run's early path); costs are |a| + |b|."""
    pairs = [(rand_seq(i % 7 + 1, i), b"") if i % 3 else (b"", rand_seq(i % 5, i)) for i in range(70)]
    want = [len(a) + len(b) for a, b in pairs]
    monkeypatch.setenv("PA_SLICE", "1")
    bt = pa.Batch(pairs)
    try:
        sh = bt.shape()
        assert sh["kernel"].startswith("pa::slice::slice_kernel<") and sh["groups"] == 0 and sh["jobs"] == 0, sh
        assert_plan(sh, [(len(a), len(b)) for a, b in pairs], sh["sliced_rows_per_lane"])
        c1, _ = bt.run()
        c2, _ = bt.run()
    finally:
        bt.close()
    assert c1.tolist() == want and np.array_equal(c1, c2)


# ---- f. content extremes -------------------------------------------------------------------------------------------------------------


def homopolymer_group(oracle):
    """X * n against Y * m for all 16 letter pairs, twice each: padding columns are code 0 (A) and padding rows have nb = 0, so a padding
    bug shows against A and T."""
    pairs, want = [], []
    for i, kind in enumerate([f"homo{x}{y}" for x in "ACGT" for y in "ACGT"] * 2):
        p, w = distinct_pairs([(COLS, ROWS)], oracle, seed=100 + i, kinds=(kind,), avoid=want)
        pairs += p
        want += w
    return pairs, want


def substring_group(oracle):
    """b a prefix, a suffix, an interior substring of a, and the other way round, at the column and row edges."""
    specs = [((n,), tuple(range(1, n))) for n in COLS if n > 2] + [(tuple(range(1, 200)), (m,)) for m in (4095, 4096, 4097, 8191, 8193, 1792, 3329)]
    return distinct_pairs(specs, oracle, seed=13, kinds=("prefix", "suffix", "sub"))


def unrelated_group(oracle):
    return distinct_pairs([(COLS, ROWS)] * 32, oracle, seed=14, kinds=("rand",))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("which", ["homopolymers", "substrings", "unrelated"])
def test_content_extremes(pa, oracle, monkeypatch, setting, which):
    make = {"homopolymers": homopolymer_group, "substrings": substring_group, "unrelated": unrelated_group}[which]
    pairs, want = cached(which, lambda: make(oracle))
    assert len(pairs) <= 32
    run_sliced(pa, monkeypatch, setting, pairs, want)


@pytest.mark.parametrize("setting", SETTINGS)
def test_identity(pa, oracle, monkeypatch, setting):
    """Identity at the column and row edges, 36 pairs in two groups (every distance 0: the one batch here without distinct distances)."""
    pairs = [(s, s) for s in (rand_seq(n, n) for n in sorted(set(COLS) | set(ROWS)))]
    run_sliced(pa, monkeypatch, setting, pairs, [0] * len(pairs), distinct=False)


# ---- g. size limits ----------------------------------------------------------------------------------------------------------------------


def _substring_pair(n, m, seed):
    """a of n bases, b its suffix of m bases (or the other way round): distance |n - m|.  The longer one ends in C, so the last columns
    (rows) count: had the last transpose block not run, they would hold code A in the column planes, T in the row planes (zero words)."""
    long_ = big_seq(max(n, m) - 1, seed) + b"C"
    short = long_[len(long_) - min(n, m) :]
    return (long_, short) if n >= m else (short, long_)


def _run_limit(pa, oracle, monkeypatch, big, extra, seed):
    """big: pairs with closed-form distances; extra: (|a| choices, |b| choices) of short pairs of the same group, against the oracle."""
    want = [d for _, _, d in big]
    pairs, w = distinct_pairs(extra, oracle, seed=seed, kinds=("rand", "mut"), avoid=want)
    pairs = [(a, b) for a, b, _ in big] + pairs
    t0 = time.perf_counter()
    run_sliced(pa, monkeypatch, 28, pairs, want + w, orders=("shuffled",))
    print(f"\n{[(len(a), len(b)) for a, b in pairs]}: {time.perf_counter() - t0:.2f} s for the batch and its two passes")


@pytest.mark.parametrize("n", [8_388_480, 8_388_481])
def test_column_limit(pa, oracle, monkeypatch, n):
    """The column transposes put (max |a| + 127) / 128 blocks in gridDim.y: 65 535 at 8 388 480, 65 536 at 8 388 481.  Shorter pairs of
    the same group put capture events across the whole width."""
    assert (n + 127) // 128 == {8_388_480: 65_535, 8_388_481: 65_536}[n]
    big = [(*_substring_pair(n, 64, 1), n - 64), (b"T" * 4_194_304, b"A" * 64, 4_194_304), (*_substring_pair(100_000, 64, 2), 100_000 - 64),
           (*_substring_pair(64, 4097, 3), 4097 - 64)]  # (the tallest: two score spans)
    short = tuple(range(32, 65))
    _run_limit(pa, oracle, monkeypatch, big, [((1,), short), ((64,), short), ((65,), short), ((129,), short), ((4097,), short)], seed=n)


@pytest.mark.parametrize("m", [16_776_704, 16_777_217])
def test_row_limit(pa, oracle, monkeypatch, m):
    """The row transpose puts (padded rows / 64 + 3) / 4 blocks in gridDim.y.  At R = 28 (strips of 1792 rows): 16 776 704 = 9362 whole
    strips = 65 534 blocks, the most R = 28 reaches below 65 535 (and the b ends on a strip boundary); 16 777 217 = 9363 strips = 65 541
    blocks.  The score kernel runs 4097 spans of rows there."""
    strips = -(-m // 1792)
    assert (strips * 1792 // 64 + 3) // 4 == {16_776_704: 65_534, 16_777_217: 65_541}[m]
    big = [(*_substring_pair(64, m, 4), m - 64), (b"G" * 60, b"C" * 5_000_000, 5_000_000)]
    short = tuple(range(32, 65))
    _run_limit(pa, oracle, monkeypatch, big, [(short, (1,)), (short, (64,)), (short, (65,)), (short, (4097,)), (short, (1792,))], seed=m)


def test_admission_bound(pa, monkeypatch):
    """|a| = 2^27 is not sliced even when forced (choose_rows_per_lane: columns are counted in 32 bits and the boundary rows addressed
    through a descriptor of n * 8 bytes); the strip kernels align it."""
    n = 1 << 27
    a, b = _substring_pair(n, 64, 5)
    monkeypatch.setenv("PA_SLICE", "28")
    bt = pa.Batch([(a, b)])
    try:
        sh = bt.shape()
        assert "sliced_rows_per_lane" not in sh and not sh["kernel"].startswith("pa::slice"), sh
        t0 = time.perf_counter()
        costs, _ = bt.run()
        print(f"\n|a| = 2^27 through {sh['kernel']}: {time.perf_counter() - t0:.2f} s")
    finally:
        bt.close()
    assert costs.tolist() == [n - 64]


# ---- h. pair counts past one encode launch -----------------------------------------------------------------------------------------------


def test_many_pairs_four_paths(pa, oracle, monkeypatch):
    """70 001 pairs of 1 .. 200 bases (the encode kernels run in launches of 32 768 pairs): bit-sliced, strip kernels, banded, traced.
    Costs against the oracle; the strip kernels only as a cross-check between the two families; every CIGAR valid at its cost."""
    count = 70_001
    rng = random.Random(15)
    pairs = []
    for i in range(count):
        a, b = gen_pair(rng.randint(1, 200), rng.choice([0.0, 0.03, 0.1, 0.3]), seed=500_000 + i)
        if rng.random() < 0.1:
            b = rand_seq(rng.randint(1, 200), 900_000 + i)
        pairs.append((a, b or b"C"))
    want = [oracle.levenshtein(a, b) for a, b in pairs]
    monkeypatch.setenv("PA_SLICE", "1")
    bt = pa.Batch(pairs)
    try:
        sh = bt.shape()
        assert sh["kernel"].startswith("pa::slice::slice_kernel<"), sh
        assert_plan(sh, [(len(a), len(b)) for a, b in pairs], sh["sliced_rows_per_lane"])
        sliced, _ = bt.run()
        again, _ = bt.run()
    finally:
        bt.close()
    assert_costs(sliced, pairs, want)
    assert np.array_equal(sliced, again)
    monkeypatch.setenv("PA_SLICE", "0")
    bt = pa.Batch(pairs)
    try:
        assert "sliced_rows_per_lane" not in bt.shape()
        strips, _ = bt.run()
        again, _ = bt.run()
    finally:
        bt.close()
    assert np.array_equal(strips, sliced) and np.array_equal(strips, again)
    monkeypatch.delenv("PA_SLICE")
    bt = pa.Batch(pairs, band=0.05)
    try:
        banded, _ = bt.run()
        again, _ = bt.run()
    finally:
        bt.close()
    assert_costs(banded, pairs, want)
    assert np.array_equal(banded, again)
    bt = pa.Batch(pairs, trace=True)
    try:
        traced, cigars, _, _ = bt.align()
        again, cigars2, _, _ = bt.align()
    finally:
        bt.close()
    assert_costs(traced, pairs, want)
    assert np.array_equal(traced, again) and cigars == cigars2
    bad = [i for i, ((a, b), c, w) in enumerate(zip(pairs, cigars, want)) if oracle.cigar_verify(c, a, b) != w]
    assert not bad, f"{len(bad)} CIGARs invalid or not at their cost, first #{bad[0]}"
