"""Seeded random cost models for every gap-affine route (tests/test_affine_random_cases.py, tests/test_gpu_affine_random.py), without a
GPU in sight.  The kernels do not read "a model": they read eleven numbers, and what they can get wrong depends on relations between
those numbers, so the models are drawn class by class, each class built (never rejected into) one such relation:

  tie         four layers: the two pieces of a direction cost the same at a drawn length L in 1 .. 20 (open_2 = open_0 + L (extend_0 -
              extend_2)); one of the pair also has linear edges that tie with piece 1 at length 1
  same        four layers: layers 2 / 3 are copies of layers 0 / 1
  dominated   four layers: piece 2 has a larger open and an extend at least as large, so it never wins
  free        the layer numbers are all distinct (eight of them, or four); in the variants after the first the pieces are ordered so
              that each of them wins somewhere
  lin_wins_1  a linear edge below open + extend of every piece of its direction
  lin_never   a linear edge above open + extend of every piece, so above every piece at every length
  no_sub      no substitution
  no_lin      no linear edge
  one_lin     exactly one linear edge
  sub_dear    sub > ins-cost(1) + del-cost(1)
  ones        every cost 1; and every cost 1 without the linear edges, so that the layers are walked
  lin_tie     two layers: open + L extend = L lin at a drawn L in 1 .. 20
  no_layers   two layers: the linear kernels (no layer at all)

Half of every class draws from 1 .. 9, half from 1 .. 60 (derived numbers, a tie's open or a dear edge, may be larger), which keeps a
pair of the plain DT oracle at a few thousand cost steps.  A name carries its index and class: m07-tie.

pairs_for(cm) is the batch of one model: five mutated pairs with |b| in 1, 15, 16, 17, 65 (16 rows to a lane), six gap pairs whose
one foreign run has the lengths at which the cheapest way to pay a gap changes hands under this very model (crossovers), as a deletion
and as an insertion, two pairs with an empty side and one unrelated pair.  ends_pairs_for(cm) are the same pairs with a as the text,
every second one with 20 + 25 random flank bytes.  long_pairs_for(cm) are two pairs with |b| = 1030 and 2060 for the chained route.

ORACLE keeps what the plain oracles say about a model, computed once a session by fill_oracle() and shared by both test modules."""
from __future__ import annotations

import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from astar_pairwise_aligner_amd import AffineCost
from tests.affine_ends_cases import SETTINGS, mutate, rand_seq

SEED = 20260
MAX_L = 40                # crossovers are looked for up to this gap length
TIE_L = 20                # a drawn tie length is at most this
FOREIGN = b"KLMN"         # bytes no sequence of ACGT holds: a run of them can only be a gap or substitutions
ROWS = (1, 15, 16, 17, 65)  # |b| of the mutated pairs: one row, R - 1, R, R + 1 and 4 R + 1 at R = 16 rows per lane
BIG = (1 << 30) - 1

FOUR_CLASSES = ("tie", "same", "dominated", "free", "lin_wins_1", "lin_never", "no_sub", "no_lin", "one_lin", "sub_dear", "ones")
TWO_CLASSES = ("free", "lin_wins_1", "lin_never", "no_sub", "no_lin", "one_lin", "sub_dear", "ones", "lin_tie", "no_layers")
FOUR_EXTRA = (("tie", 2), ("free", 2))  # 2 * 11 + 2 = 24 models
KINDS4 = ("ins", "del", "ins", "del")


def class_of(name: str) -> str:
    return name.split("-", 1)[1]


def _r(rng, lo, hi) -> int:
    return int(rng.integers(lo, hi + 1))


def _h(variant: int) -> int:
    """The range of a variant: even ones draw from 1 .. 9, odd ones from 1 .. 60."""
    return 60 if variant % 2 else 9


def _two_pieces(rng, H):
    """(open_0, extend_0, open_2, extend_2) with piece 2 the dearer to open and the cheaper to extend: each wins somewhere."""
    e0 = _r(rng, 2, H)
    e2 = _r(rng, 1, e0 - 1)
    o0 = _r(rng, 1, H)
    return o0, e0, o0 + _r(rng, 1, H), e2


def _tied_pieces(rng, H):
    """Two pieces that cost the same at a drawn length L: open_2 = open_0 + L (extend_0 - extend_2), at most 60 + 20 * 45."""
    e0 = _r(rng, 2, H)
    d = _r(rng, 1, min(e0 - 1, 45))
    o0 = _r(rng, 1, H)
    return o0, e0, o0 + _r(rng, 1, TIE_L) * d, e0 - d


def _four(sub, ins, dl, pi, pd) -> AffineCost:
    return AffineCost(sub, ins, dl, [("ins", pi[0], pi[1]), ("del", pd[0], pd[1]), ("ins", pi[2], pi[3]), ("del", pd[2], pd[3])])


def _build4(cls: str, variant: int, rng) -> AffineCost:
    H = _h(variant)
    sub = _r(rng, 1, H)
    pi, pd = _two_pieces(rng, H), _two_pieces(rng, H)
    mid = lambda p: p[3] + _r(rng, 1, H)  # noqa: E731  a linear edge steeper than the flattest piece: long gaps go to a layer
    first = lambda p: min(p[0] + p[1], p[2] + p[3])  # noqa: E731  the pieces' cost of one byte
    if cls == "tie":
        pi, pd = _tied_pieces(rng, H), _tied_pieces(rng, H)
        if variant % 2:
            return _four(sub, pi[0] + pi[1], pd[0] + pd[1], pi, pd)
        return _four(sub, None, None, pi, pd)
    if cls == "same":
        pi, pd = pi[:2] * 2, pd[:2] * 2
        return _four(sub, pi[1] + _r(rng, 1, H), None, pi, pd) if variant % 2 else _four(sub, None, None, pi, pd)
    if cls == "dominated":
        up = lambda p: (p[0], p[1], p[0] + _r(rng, 1, H), p[1] + (_r(rng, 1, H) if variant % 2 else 0))  # noqa: E731
        return _four(sub, None, None, up(pi), up(pd))
    if cls == "free":
        v = [int(x) + 1 for x in rng.permutation(H)[:8]]
        if variant:  # per direction: the flattest piece is the dearest to open
            si, sd = sorted(v[:4]), sorted(v[4:])
            return _four(sub, None, None, (si[2], si[1], si[3], si[0]), (sd[2], sd[1], sd[3], sd[0]))
        return _four(sub, None, None, (v[0], v[1], v[4], v[5]), (v[2], v[3], v[6], v[7]))
    if cls == "lin_wins_1":
        return _four(sub, _r(rng, pi[3] + 1, first(pi) - 1), _r(rng, pd[3] + 1, first(pd) - 1), pi, pd)  # and above the flattest extend
    if cls == "lin_never":
        return _four(sub, max(pi[0] + pi[1], pi[2] + pi[3]) + _r(rng, 1, H), max(pd[0] + pd[1], pd[2] + pd[3]) + _r(rng, 1, H), pi, pd)
    if cls == "no_sub":
        return _four(None, mid(pi), mid(pd), pi, pd) if variant % 2 else _four(None, None, None, pi, pd)
    if cls == "no_lin":
        return _four(sub, None, None, pi, pd)
    if cls == "one_lin":
        return _four(sub, None, mid(pd), pi, pd) if variant % 2 else _four(sub, mid(pi), None, pi, pd)
    if cls == "sub_dear":
        ins, dl = (mid(pi), mid(pd)) if variant % 2 else (None, None)
        one = min(first(pi), ins or first(pi)) + min(first(pd), dl or first(pd))
        return _four(one + _r(rng, 1, H), ins, dl, pi, pd)
    if cls == "ones":
        return _four(1, None, None, (1, 1, 1, 1), (1, 1, 1, 1)) if variant % 2 else _four(1, 1, 1, (1, 1, 1, 1), (1, 1, 1, 1))
    raise ValueError(cls)


def _two(sub, ins, dl, li, ld) -> AffineCost:
    return AffineCost(sub, ins, dl, [("ins", *li), ("del", *ld)])


def _build2(cls: str, variant: int, rng) -> AffineCost:
    H = _h(variant)
    sub = _r(rng, 1, H)
    li, ld = (_r(rng, 1, H), _r(rng, 1, H)), (_r(rng, 1, H), _r(rng, 1, H))
    mid = lambda p: p[1] + _r(rng, 1, H)  # noqa: E731  steeper than the layer: long gaps go to the layer
    if cls == "free":
        v = [int(x) + 1 for x in rng.permutation(H)[:4]]
        return _two(sub, None, None, (v[0], v[1]), (v[2], v[3]))
    if cls == "lin_wins_1":
        li, ld = (li[0] + 1, li[1]), (ld[0] + 1, ld[1])
        return _two(sub, _r(rng, li[1] + 1, sum(li) - 1), _r(rng, ld[1] + 1, sum(ld) - 1), li, ld)  # and above the extend
    if cls == "lin_never":
        return _two(sub, sum(li) + _r(rng, 1, H), sum(ld) + _r(rng, 1, H), li, ld)
    if cls == "no_sub":
        return _two(None, mid(li), mid(ld), li, ld) if variant % 2 else _two(None, None, None, li, ld)
    if cls == "no_lin":
        return _two(sub, None, None, li, ld)
    if cls == "one_lin":
        return _two(sub, None, mid(ld), li, ld) if variant % 2 else _two(sub, mid(li), None, li, ld)
    if cls == "sub_dear":
        ins, dl = (mid(li), mid(ld)) if variant % 2 else (None, None)
        return _two(min(sum(li), ins or sum(li)) + min(sum(ld), dl or sum(ld)) + _r(rng, 1, H), ins, dl, li, ld)
    if cls == "ones":
        return _two(1, None, None, (1, 1), (1, 1)) if variant % 2 else _two(1, 1, 1, (1, 1), (1, 1))
    if cls == "lin_tie":  # open + L extend = L lin: lin = extend + d, open = L d
        def tied():
            e, d = _r(rng, 1, H), _r(rng, 1, min(H, 45))
            return e + d, (_r(rng, 1, TIE_L) * d, e)
        (ins, li), (dl, ld) = tied(), tied()
        return _two(sub, ins, dl, li, ld)
    if cls == "no_layers":
        return AffineCost(None if variant % 2 else sub, _r(rng, 1, H), _r(rng, 1, H))
    raise ValueError(cls)


def _models(classes, extra, build, seed):
    rng = np.random.default_rng(seed)
    plan = [(c, v) for c in classes for v in (0, 1)] + list(extra)
    return {"m%02d-%s" % (k, c): build(c, v, rng) for k, (c, v) in enumerate(plan)}


def models2(seed: int = SEED) -> dict:
    """name -> AffineCost for AffineBatch: two of every class of TWO_CLASSES."""
    return _models(TWO_CLASSES, (), _build2, [seed, 2])


def models4(seed: int = SEED) -> dict:
    """name -> AffineCost for Affine4Batch: two of every class of FOUR_CLASSES, a third tie and a third free."""
    return _models(FOUR_CLASSES, FOUR_EXTRA, _build4, [seed, 4])


def models(kind: int, seed: int = SEED) -> dict:
    return models4(seed) if kind == 4 else models2(seed)


def lifted(cm: AffineCost) -> AffineCost:
    """A two-layer model (or one without layers) as a four-layer one whose added layers can never win: a larger open and a larger
    extend than the piece they stand next to, or than the linear edge where there is no piece."""
    if cm.layers:
        return AffineCost(cm.sub, cm.ins, cm.del_, list(cm.layers) + [(k, o + 7, e + 3) for k, o, e in cm.layers])
    return AffineCost(cm.sub, cm.ins, cm.del_, [(k, lin + 3, lin + 2) for _ in range(2) for k, lin in (("ins", cm.ins), ("del", cm.del_))])


def swapped(cm: AffineCost, what: str, layers) -> AffineCost:
    """`cm` with the extends ("extend"), the opens ("open") or both numbers ("layer") of the layer pairs in `layers` exchanged."""
    lay = [list(x) for x in cm.layers]
    for s, t in layers:
        for q in {"extend": (2,), "open": (1,), "layer": (1, 2)}[what]:
            lay[s][q], lay[t][q] = lay[t][q], lay[s][q]
    return AffineCost(cm.sub, cm.ins, cm.del_, [tuple(x) for x in lay])


SWAPS = (((0, 2),), ((1, 3),), ((0, 2), (1, 3)))


def free_model(seed: int = SEED) -> AffineCost:
    """The free four-layer model of the layer-swap tests: the first whose pieces each win somewhere, in both directions."""
    return next(cm for n, cm in models4(seed).items() if class_of(n) == "free" and crossovers(cm, "ins") and crossovers(cm, "del"))


# ---- what a gap costs under a model

def gap_options(cm, direction: str):
    """[(open, slope)] of every way to pay a gap of one direction: the linear edge (open 0) first, then the pieces in layer order."""
    lin = cm.ins if direction == "ins" else cm.del_
    return ([(0, lin)] if lin is not None else []) + [(o, e) for k, o, e in cm.layers if k == direction]


def gap_cost(cm, direction: str, L: int) -> int:
    return 0 if L == 0 else min(o + L * e for o, e in gap_options(cm, direction))


def crossovers(cm, direction: str):
    """The lengths L in 1 .. MAX_L at which a way to pay the gap is among the cheapest that was not at L - 1 (ways with the same two
    numbers are one way); and 1 where several ways tie there."""
    opts = sorted(set(gap_options(cm, direction)))
    out, prev = [], None
    for L in range(1, MAX_L + 1):
        costs = [o + L * e for o, e in opts]
        best = {k for k, c in enumerate(costs) if c == min(costs)}
        if (L == 1 and len(best) > 1) or (L > 1 and not best <= prev):
            out.append(L)
        prev = best
    return out


def tie_length(cm, direction: str):
    """The length at which the two pieces of a direction cost the same, None where there is no such whole length."""
    (o0, e0), (o2, e2) = [(o, e) for k, o, e in cm.layers if k == direction]
    if e0 == e2 or (o2 - o0) % (e0 - e2) or (o2 - o0) // (e0 - e2) < 1:
        return None
    return (o2 - o0) // (e0 - e2)


def gap_lengths(cm, direction: str):
    """Three run lengths for one direction: the crossovers themselves first, then the lengths after and before them; 1, 2 and 20
    where the model has no crossover (or not three lengths around it)."""
    cross = crossovers(cm, direction)
    cand = cross + [L + 1 for L in cross] + [L - 1 for L in cross] + [1, 2, 20]
    out = []
    for L in cand:
        if L >= 1 and L not in out:
            out.append(L)
    return sorted(out[:3])


# ---- the pairs

def _rng(cm, seed, salt):
    nums = [cm.sub, cm.ins, cm.del_] + [x for _, o, e in cm.layers for x in (o, e)]
    return np.random.default_rng([seed, salt] + [0 if v is None else int(v) for v in nums])


def _mutated(rng, y: bytes, rate: float) -> bytes:
    """mutate(y) with at least one change: an unchanged copy gets one substitution."""
    x = mutate(rng, y, rate)
    if x == y:
        p = _r(rng, 0, len(y) - 1)
        x = y[:p] + (b"A" if y[p:p + 1] != b"A" else b"C") + y[p + 1:]
    return x


def gap_pairs(cm, seed: int = SEED):
    """[(a, b, direction, L)]: a 70-byte sequence against itself with L foreign bytes after byte 33, the run on a's side (a deletion)
    and on b's (an insertion), L of gap_lengths."""
    rng = _rng(cm, seed, 1)
    out = []
    for direction in ("del", "ins"):
        for L in gap_lengths(cm, direction):
            x = rand_seq(rng, 70)
            y = x[:33] + rand_seq(rng, L, FOREIGN) + x[33:]
            out.append((y, x, direction, L) if direction == "del" else (x, y, direction, L))
    return out


def pairs_for(cm, seed: int = SEED):
    """The 14 pairs of one model, |a| <= 130: 0 .. 4 mutated at 10 to 20 %, 5 .. 10 the gap pairs, 11 and 12 with an empty side, 13
    unrelated."""
    rng = _rng(cm, seed, 0)
    pairs = []
    for m in ROWS:
        y = rand_seq(rng, m)
        pairs.append((_mutated(rng, y, 0.10 + 0.10 * rng.random()), y))
    pairs += [(a, b) for a, b, _, _ in gap_pairs(cm, seed)]
    x = rand_seq(rng, 7)
    pairs += [(x, b""), (b"", x[:5]), (rand_seq(rng, 40), rand_seq(rng, 33))]
    assert all(len(a) <= 130 for a, _ in pairs)
    return pairs


def ends_pairs_for(cm, seed: int = SEED):
    """pairs_for with a as the text; every second pair's text gets 20 random bytes in front and 25 behind."""
    rng = _rng(cm, seed, 2)
    return [(rand_seq(rng, 20) + a + rand_seq(rng, 25), b) if p % 2 else (a, b) for p, (a, b) in enumerate(pairs_for(cm, seed))]


LONG_M = (1030, 2060)
STRIP = 1024  # rows of a chained strip


def long_pairs_for(cm, seed: int = SEED):
    """Two pairs with |b| = 1030 and 2060 and |a| <= 70: b holds one foreign run of a crossover length (the larger two of
    gap_lengths(cm, "ins"), so at least 2 bytes) that covers row 1024 and ends at or before row 1027; a is a mutated copy of the 40 rows before the run and
    the rows after it (3 and 25 of them)."""
    rng = _rng(cm, seed, 3)
    out = []
    for m, L, after in zip(LONG_M, gap_lengths(cm, "ins")[1:], (3, 25)):
        last = STRIP + min(3, L - 1)  # the run covers rows last - L + 1 .. last
        first = last - L + 1
        assert first <= STRIP <= last and last + 3 <= LONG_M[0]
        y = rand_seq(rng, m - L)
        b = y[:first - 1] + rand_seq(rng, L, FOREIGN) + y[first - 1:]
        a = _mutated(rng, y[first - 41:first - 1] + y[first - 1:first - 1 + after], 0.1)[:70]
        assert len(b) == m
        out.append((a, b))
    return out


# ---- the oracles' word on one model, once a session

ORACLE = {}  # (kind, name) -> oracle_model(kind, name)


def oracle_model(kind: int, name: str, seed: int = SEED) -> dict:
    """Everything the plain oracles say about one model at the default pairs:
      nw, nw_raw     [(cost, CIGAR)] and the raw ops of the plain DP over pairs_for
      dt, dt_raw     [(cost, CIGAR)] of the plain DT without a bound (raw ops: four layers only)
      ends, dt_ends  {(free_start, free_end): [(cost, CIGAR, start, end)]} of the ends-free DP and DT over ends_pairs_for
      long           [(cost, CIGAR)] of the plain DP over long_pairs_for
      lift_nw, lift_dt   two layers only: nw and dt by the four-layer oracles under lifted(cm)"""
    from tests import affine4_plain as a4
    from tests import affine_plain as ap
    from tests.affine4_dt_plain import affine4_dt
    from tests.affine4_ends_plain import affine4_ends
    from tests.affine_dt_ends_plain import affine_dt_ends
    from tests.affine_dt_plain import affine_dt
    from tests.affine_ends_plain import affine_ends

    cm = models(kind, seed)[name]
    pairs, epairs, longs = pairs_for(cm, seed), ends_pairs_for(cm, seed), long_pairs_for(cm, seed)
    nw = a4.affine4_nw if kind == 4 else ap.affine_nw
    ends = affine4_ends if kind == 4 else affine_ends
    out = {"nw": [nw(x, y, cm) for x, y in pairs], "nw_raw": [nw(x, y, cm, raw=True)[1] for x, y in pairs],
           "long": [nw(x, y, cm) for x, y in longs], "ends": {}, "dt_ends": {}}
    if kind == 2:
        up = lifted(cm)
        out["lift_nw"] = [a4.affine4_nw(x, y, up) for x, y in pairs]
        out["lift_dt"] = [affine4_dt(x, y, up, BIG)[:2] for x, y in pairs]
    if kind == 4:
        out["dt"] = [affine4_dt(x, y, cm, BIG)[:2] for x, y in pairs]
        out["dt_raw"] = [affine4_dt(x, y, cm, BIG, raw=True)[1] for x, y in pairs]
    else:
        out["dt"] = [affine_dt(x, y, cm, BIG) for x, y in pairs]
    for fs, fe in SETTINGS:
        res = [ends(x, y, cm, fs, fe) for x, y in epairs]
        out["ends"][fs, fe] = [(c, g, st, en) for c, st, en, g, _ in res]
        if kind == 4:
            out["dt_ends"][fs, fe] = [affine4_dt(x, y, cm, BIG, fs, fe) for x, y in epairs]
        else:
            out["dt_ends"][fs, fe] = [(c, g, st, en) for c, st, en, g in (affine_dt_ends(x, y, cm, BIG, fs, fe) for x, y in epairs)]
    return out


def fill_oracle(workers: int = 8) -> dict:
    """ORACLE for every model of both kinds that it does not hold yet, a model to a fresh worker process (started, not forked: they
    share nothing with this process)."""
    keys = [(kind, name) for kind in (2, 4) for name in models(kind) if (kind, name) not in ORACLE]
    if keys:
        with ProcessPoolExecutor(max_workers=min(workers, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as pool:
            ORACLE.update(zip(keys, pool.map(oracle_model, *zip(*keys))))
    return ORACLE
