"""The models and pairs of the heavy-cost tests (tests/test_affine_heavy_cases.py, tests/test_gpu_affine_heavy.py), without a GPU in sight:
cost components up to 1000, the largest the batch types take, and totals next to 2^30, the bound their length check keeps every
reachable cost below.  On the diagonal-transition routes the cost magnitude is the shape of the computation: the ring has `largest
edge + 1` slots, whole fronts are empty, and a segment keeps `largest edge` checkpoint rows.  The pairs are the smallest that still get
there, because the plain DT oracle pays for every cost step: a DT pair stays at or below about 120 bytes."""
from __future__ import annotations

import numpy as np

from astar_pairwise_aligner_amd import AffineCost
from tests.affine_ends_cases import mutate, rand_seq

LIMIT = 1 << 30

# Two layers (AffineBatch).  E, the largest single edge, is 1000 under every one of them.
MODELS = {
    "flat_1000": AffineCost.affine(1000, 1000, 1000),                      # every cost a multiple of 1000: 999 fronts of 1000 are empty
    "coprime": AffineCost.affine_asymmetric(997, 1000, 991, 983, 1000),    # many residues; E is an open on one side, an extend on the other
    "cheap_sub": AffineCost.affine(1, 1000, 1),                            # dense fronts, a ring of 1001 live slots, the layer opens at s = 1000
    "linear_heavy": AffineCost.linear(1000, 999),                          # no layers: the AFF = false kernels
    "no_sub_heavy": AffineCost(None, 1000, 1000),                          # sub absent (kInf) next to large real costs
    "crossover": AffineCost.linear_affine(500, 700, 1000, 300),            # the linear indel wins up to length 2 (1400 < 1600), the layer from 3 (1900 < 2100)
}

# Four layers (Affine4Batch).
MODELS4 = {
    # the two pieces tie at length 3 (100 + 3 * 700 = 1000 + 3 * 400 = 2200): the layer order decides; piece 2 wins above that
    "double_heavy": AffineCost.double_affine(900, 100, 700, 1000, 400),
    # piece 2 wins from length 2 (insert) and 3 (delete); one extend at 1000, and a linear delete that wins at length 1 (850 < 900)
    "asymmetric_heavy": AffineCost(800, None, 850, [("ins", 50, 1000), ("del", 300, 600), ("ins", 900, 450), ("del", 1000, 350)]),
    # no substitution, no linear edge; piece 2 wins from length 3 (1000 + 3 * 500 < 200 + 3 * 800)
    "no_sub4_heavy": AffineCost(None, None, None, [("ins", 200, 800), ("del", 200, 800), ("ins", 1000, 500), ("del", 1000, 500)]),
    # cheap_sub with four layers: dense fronts, no layer opens before s = 998; the main ring of the DT route has 1001 live slots while
    # the layer rings have 2, 2, 3 and 4 and wrap hundreds of times for each wrap of the main one.  Both pieces cost 1001 at length 1
    # (1000 + 1 = 999 + 2 = 998 + 3: the layer order decides); piece 1 wins above that
    "dense4": AffineCost(1, None, None, [("ins", 1000, 1), ("del", 1000, 1), ("ins", 999, 2), ("del", 998, 3)]),
    # E = 1000 comes from the main layer's own edges (sub 1000, linear 999 / 998), every open is below 300 and an extend reaches 1000:
    # layer rings of 1001, 521, 781 and 301 slots.  The linear insert wins at length 1 (999 < 299 + 780), layer 2 from 2; layer 0 never
    # wins; layer 1 wins a deletion of 1 (530 < 599), layer 3 from 2; the linear delete never wins
    "main_edge4": AffineCost(1000, 999, 998, [("ins", 290, 1000), ("del", 10, 520), ("ins", 299, 780), ("del", 299, 300)]),
}

FOREIGN = b"NRYK"  # bytes the flanks do not have: a gap of them has one best place


def cut_layers(cm, keep):
    """`cm` with only its first `keep` layers."""
    return AffineCost(cm.sub, cm.ins, cm.del_, cm.layers[:keep])


# ---- the diagonal-transition pairs

def dt_small(seed=41):
    """Cost 0, one substitution, one inserted and one deleted byte: costs below, on and just above E = 1000 (a byte of gap under
    flat_1000 costs 2000, under cheap_sub 1001, a substitution under cheap_sub 1); both sequences empty and one of them empty."""
    rng = np.random.default_rng(seed)
    x = rand_seq(rng, 70)
    sub1 = x[:30] + (b"A" if x[30:31] != b"A" else b"C") + x[31:]
    return [(x, x), (x, sub1), (x, x[:40] + b"N" + x[40:]), (x, x[:20] + x[21:]), (b"", b""), (x[:3], b""), (b"", x[:2])]


def dt_ladder(seed=42):
    """One 60-byte sequence against itself with 1 .. 12 substitutions (tests/affine_dt_seg_cases.ladder): costs sub, 2 sub, .. 12 sub."""
    rng = np.random.default_rng(seed)
    x = rand_seq(rng, 60, b"AC")
    pairs, y = [], bytearray(x)
    for q in range(12):
        y[3 + 5 * q - (q % 2)] = ord("G")
        pairs.append((x, bytes(y)))
    return pairs


GAP = 20


def dt_gap(seed=43):
    """Two matching flanks of 25 and 20 bytes around GAP foreign bytes, as a deletion and as an insertion: the walk stays in a layer
    across GAP extends, 21 000 costs under flat_1000."""
    rng = np.random.default_rng(seed)
    left, right, mid = rand_seq(rng, 25), rand_seq(rng, 20), rand_seq(rng, GAP, FOREIGN)
    a, b = left + mid + right, left + right
    return [(a, b), (b, a)]


def dt_runs(seed=44):
    """One pair with foreign gaps of 1, 2, 3 and 4 bytes, 14 matching bytes apart, insertions and deletions in turn: the lengths at
    which the linear edge, the first and the second piece take over from each other under `crossover` and the four-layer models."""
    rng = np.random.default_rng(seed)
    x = rand_seq(rng, 70)
    a = x[:14] + x[14:28] + rand_seq(rng, 2, FOREIGN) + x[28:42] + x[42:56] + rand_seq(rng, 4, FOREIGN) + x[56:]
    b = x[:14] + rand_seq(rng, 1, FOREIGN) + x[14:28] + x[28:42] + rand_seq(rng, 3, FOREIGN) + x[42:56] + x[56:]
    return [(a, b)]


def dt_mutated(seed=45):
    """Five pairs of 60 .. 120 bp at 8 .. 10 %."""
    rng = np.random.default_rng(seed)
    pairs = []
    for n, rate in ((60, 0.10), (75, 0.08), (90, 0.10), (105, 0.09), (120, 0.08)):
        x = rand_seq(rng, n)
        pairs.append((x, mutate(rng, x, rate)))
    return pairs


FAR = 70


def dt_far(seed=46, far=FAR, first=30):
    """|a| - |b| = +-far (70) around a core of 12 bytes: the end diagonal lies outside the first 64 lanes while a cost step reaches
    nowhere.  The surplus is foreign and split first / far - first (30 / 40) around the core: two gaps, 72 000 costs under flat_1000."""
    rng = np.random.default_rng(seed)
    core = rand_seq(rng, 12)
    long_ = rand_seq(rng, first, FOREIGN) + core + rand_seq(rng, far - first, FOREIGN)
    return [(long_, core), (core, long_)]


def dt_cases():
    return dict(dt_small=dt_small(), dt_ladder=dt_ladder(), dt_gap=dt_gap(), dt_runs=dt_runs(), dt_mutated=dt_mutated(), dt_far=dt_far())


FAR4 = 65  # the smallest surplus with |a| - |b| above 64: the end diagonal stays outside the first wavefront's first pass


def dt4_cases():
    """The lists of the four-layer DT tests: dt_cases() with every second rung of the ladder (2, 4 .. 12 substitutions) and a far pair
    of surplus FAR4 = 65, split 25 / 40 (12 + 65 against 12): the plain four-layer DT pays for five layers a cost step."""
    return dict(dt_cases(), dt_ladder=dt_ladder()[1::2], dt_far=dt_far(far=FAR4, first=25))


SEG_CASES = ("dt_small", "dt_ladder", "dt_gap", "dt_mutated")  # the batch of the segmented route's test


DT_ORACLE = {}  # (model, case) -> [(cost, CIGAR)]: the plain DT's results, shared by every test module of one session


def dt_oracle_case(name, case):
    """[(cost, CIGAR)] of dt_cases()[case] under MODELS[name] by the plain DT without a bound, computed once."""
    from tests.affine_dt_plain import affine_dt

    if (name, case) not in DT_ORACLE:
        DT_ORACLE[name, case] = [affine_dt(x, y, MODELS[name], LIMIT - 1) for x, y in dt_cases()[case]]
    return DT_ORACLE[name, case]


def dt_oracle(name):
    """{case: [(cost, CIGAR)]} of every case under MODELS[name]."""
    return {c: dt_oracle_case(name, c) for c in dt_cases()}


DT4_ORACLE = {}  # (model, case) -> [(cost, CIGAR)] of the plain four-layer DT, shared like DT_ORACLE


def dt4_oracle_case(name, case):
    """[(cost, CIGAR)] of dt4_cases()[case] under MODELS4[name] by the plain four-layer DT without a bound, computed once."""
    from tests.affine4_dt_plain import affine4_dt

    if (name, case) not in DT4_ORACLE:
        DT4_ORACLE[name, case] = [affine4_dt(x, y, MODELS4[name], LIMIT - 1)[:2] for x, y in dt4_cases()[case]]
    return DT4_ORACLE[name, case]


DT4_ENDS_MODELS = ("double_heavy", "dense4", "main_edge4")  # the models of the ends-free and the pair-by-pair four-layer DT tests


def dt4_ends_oracle(name, fs, fe):
    """[(cost, CIGAR, start, end)] of dt_planted() under MODELS4[name] by the plain ends-free four-layer DT, computed once."""
    from tests.affine4_dt_plain import affine4_dt

    if (name, fs, fe) not in DT4_ORACLE:
        DT4_ORACLE[name, fs, fe] = [affine4_dt(x, y, MODELS4[name], LIMIT - 1, fs, fe) for x, y in dt_planted()]
    return DT4_ORACLE[name, fs, fe]


WIDE_N = 300


def dt4_wide(seed=50):
    """Four pairs of about 300 bytes at 10 % for the dense model: a cost of 1130 or more there pays for gaps of 131 bytes each way,
    so the mean W of the batch at its largest cost is above 256 and its blocks are four wavefronts wide."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(4):
        x = rand_seq(rng, WIDE_N)
        pairs.append((x, mutate(rng, x, 0.10)))
    return pairs


def dt4_wide_oracle():
    from tests.affine4_dt_plain import affine4_dt

    if "wide" not in DT4_ORACLE:
        DT4_ORACLE["wide"] = [affine4_dt(x, y, MODELS4["dense4"], LIMIT - 1)[:2] for x, y in dt4_wide()]
    return DT4_ORACLE["wide"]


def fill_dt4_oracle(workers=8):
    """DT4_ORACLE for every (model, case) of the four-layer DT tests, the ends-free lists and the wide batch that it does not hold
    yet: about 150 s of the plain oracle in one process, so fresh worker processes take a key each (started, not forked)."""
    import multiprocessing
    import os
    from concurrent.futures import ProcessPoolExecutor

    keys = [(name, c) for name in MODELS4 for c in dt4_cases() if (name, c) not in DT4_ORACLE]
    ends = [(name, fs, fe) for name in DT4_ENDS_MODELS for fs in (False, True) for fe in (False, True) if (name, fs, fe) not in DT4_ORACLE]
    if keys or ends or "wide" not in DT4_ORACLE:
        with ProcessPoolExecutor(max_workers=min(workers, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as pool:
            wide = pool.submit(dt4_wide_oracle)
            res = list(pool.map(dt4_oracle_case, *zip(*keys))) if keys else []
            eres = list(pool.map(dt4_ends_oracle, *zip(*ends))) if ends else []
            DT4_ORACLE["wide"] = wide.result()
        DT4_ORACLE.update(zip(keys, res))
        DT4_ORACLE.update(zip(ends, eres))
    return DT4_ORACLE


def dt_planted(seed=47):
    """(text, pattern) for the ends-free DT route: patterns planted at 10 % (tests/affine_ends_cases.planted) in texts of 30 .. 100
    bytes, a hit that is the text's suffix, one that is its prefix, a text shorter than the pattern and an empty one.  The flanks are
    8 to 10 bytes in all: with both ends fixed they are deleted, at up to 1000 cost steps of the plain oracle a byte."""
    from tests.affine_ends_cases import planted

    rng = np.random.default_rng(seed)
    pairs = [planted(rng, n, rand_seq(rng, m)) for n, m in ((30, 20), (40, 30), (100, 90))]
    y = rand_seq(rng, 30)
    pairs += [(rand_seq(rng, 8) + y, y), (y + rand_seq(rng, 8), y[:14] + y[15:]), (y[:24], y), (b"", y[:3])]
    return pairs


# ---- the strip kernels' pairs

EDGE_N = (1, 63, 64, 65, 130)
EDGE_ROTATIONS = (0, 2)
GAP_RUN = 30


def edge_m(R):
    return (1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 128 * R + 1)


def _gap_pair(rng, R, kind):
    """A pair with one run of GAP_RUN foreign bytes aimed at an edge, and its aim: ("I", 64 R) for an insertion run that is open at
    row 64 R, ("D", 64) for a deletion run that is open at column 64.  The aimed side keeps a length of the edge lists; where b is
    much longer than a, the rest of b is inserted before and after the window that a matches."""
    S = 64 * R
    gap = rand_seq(rng, GAP_RUN, FOREIGN)
    if kind in (0, 4):  # |b| = 128 R + 1, |a| = 130 or 63: flanks of |a| / 2 around rows S - 15 .. S + 15
        n = 130 if kind == 0 else 63
        y = rand_seq(rng, 128 * R + 1 - GAP_RUN)
        j0 = S - GAP_RUN // 2
        return (y[j0 - (n + 1) // 2:j0] + y[j0:j0 + n // 2], y[:j0] + gap + y[j0:]), ("I", S)
    if kind == 2:       # |b| = 64 R + 1, |a| = 130: a is b's head, the run b's last 30 rows, which the rows before it join in one insertion
        y = rand_seq(rng, S + 1 - GAP_RUN)
        return (y[:130], y + gap), ("I", S)
    if kind == 1:       # |a| = 130: the run lies over columns 49 .. 79
        x = rand_seq(rng, 130 - GAP_RUN)
        return (x[:49] + gap + x[49:], x), ("D", 64)
    x = rand_seq(rng, 65 - GAP_RUN)  # |a| = 65: the run is a's last 30 columns, 35 .. 65
    return (x + gap, x), ("D", 64)


def nw_edges_aimed(R, seed=48):
    """[(a, b, aim)]: |b| of edge_m(R) against |a| of EDGE_N, the k-th |b| with EDGE_N[(k + rot) % 5] for the rotations
    EDGE_ROTATIONS (tests/affine_ends_cases.edge_pairs), odd pairs mutated windows of b, even ones unrelated; after every two of
    them a gap pair of _gap_pair, so that every third pair of the list has a 30-byte foreign run across the 64 R row or across
    column 64.  aim is None for the shape pairs."""
    rng = np.random.default_rng(seed)
    shapes = []
    for rot in EDGE_ROTATIONS:
        for k, m in enumerate(edge_m(R)):
            n = EDGE_N[(k + rot) % len(EDGE_N)]
            y = rand_seq(rng, m)
            if len(shapes) % 2:
                off = int(rng.integers(0, max(m - n, 0) + 1))
                x = (mutate(rng, y[off:off + n], 0.1) + rand_seq(rng, n))[:n]
            else:
                x = rand_seq(rng, n)
            shapes.append((x, y, None))
    out = []
    for q in range(0, len(shapes), 2):
        out += shapes[q:q + 2]
        pair, aim = _gap_pair(rng, R, (q // 2) % 5)
        out.append((*pair, aim))
    return out


def nw_edges(R, seed=48):
    return [(x, y) for x, y, _ in nw_edges_aimed(R, seed)]


def runs_of(cigar, op):
    """[((i, j) before, (i, j) after)] of every run of `op` in the path (tests/test_gpu_affine4_tiled.runs_of)."""
    from tests.affine_plain import cigar_elems

    out, i, j = [], 0, 0
    for k, o in cigar_elems(cigar):
        di, dj = (k, k) if o in "=X" else (0, k) if o == "I" else (k, 0)
        if o == op:
            out.append(((i, j), (i + di, j + dj)))
        i, j = i + di, j + dj
    return out


def aim_is_met(cigar, aim):
    """The path has a run of the aim's op, at least GAP_RUN long, that starts before the aim's row / column and ends after it."""
    op, at = aim
    axis = 1 if op == "I" else 0
    return any(p0[axis] < at < p1[axis] and p1[axis] - p0[axis] >= GAP_RUN for p0, p1 in runs_of(cigar, op))


# ---- totals next to 2^30

THIN_MODELS = {
    "linear_1000": AffineCost.linear(1000, 1000),
    "affine_1_999": AffineCost.affine(1000, 1, 999),
}
# the cheapest layer is (1, 999) on both sides; the other piece is the same line (any other with open + extend <= 1000 would be cheaper
# somewhere), and the linear edges at 1000 tie with it at length 1
THIN_MODELS4 = {
    "four_1_999": AffineCost(1000, 1000, 1000, [("ins", 1, 999), ("del", 1, 999), ("ins", 1, 999), ("del", 1, 999)]),
}


def create_max_edge(cm) -> int:
    """max edge as the create calls compute it: max(sub, ins, del, open + extend per layer)."""
    return max([v for v in (cm.sub, cm.ins, cm.del_) if v is not None] + [o + e for _, o, e in cm.layers])


def thin_n(cm) -> int:
    """N, the largest |a| + |b| the create call accepts: (N + 1) max_edge < 2^30 <= (N + 2) max_edge."""
    return (LIMIT - 1) // create_max_edge(cm) - 1


def thin_k(N) -> int:
    return N // 2 + 7


def thin_limit(cm, N=None):
    """The four thin pairs of total length N (default thin_n(cm)): all of a deleted, all of b inserted, and a single C matched between
    two gaps of k and N - 2 - k bytes, both ways round."""
    N = thin_n(cm) if N is None else N
    k = thin_k(N)
    long_ = b"A" * k + b"C" + b"A" * (N - 2 - k)
    return [(b"A" * N, b""), (b"", b"A" * N), (long_, b"C"), (b"C", long_)]


def gap_w(L, lin, pieces) -> int:
    """The cost of one gap of length L: the cheapest of the linear edge (None: absent) and the (open, extend) pieces."""
    if L == 0:
        return 0
    return min([o + L * e for o, e in pieces] + ([L * lin] if lin is not None else []))


def thin_expected(cm, N=None):
    """[(cost, CIGAR)] of thin_limit(cm, N) in closed form: one gap of N, or kD 1= (N-2-k)D (a count of 1 is not printed).  A
    substitution of the C's partner would save no gap byte (sub + w(N - 2) against w(k) + w(N - 2 - k) with sub >= 1000 > an open)."""
    N = thin_n(cm) if N is None else N
    k = thin_k(N)
    wi = lambda L: gap_w(L, cm.ins, [(o, e) for kind, o, e in cm.layers if kind == "ins"])   # noqa: E731
    wd = lambda L: gap_w(L, cm.del_, [(o, e) for kind, o, e in cm.layers if kind == "del"])  # noqa: E731
    return [(wd(N), f"{N}D"), (wi(N), f"{N}I"), (wd(k) + wd(N - 2 - k), f"{k}D={N - 2 - k}D"), (wi(k) + wi(N - 2 - k), f"{k}I={N - 2 - k}I")]


def ordinary(seed=49):
    """Three ordinary small pairs to share a batch with the thin ones."""
    rng = np.random.default_rng(seed)
    x, y = rand_seq(rng, 40), rand_seq(rng, 300)
    return [(x, mutate(rng, x, 0.1)), (mutate(rng, y, 0.08), y), (rand_seq(rng, 25), rand_seq(rng, 31))]
