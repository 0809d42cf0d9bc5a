"""A plain restatement of A*PA2's outer loop for tests/test_band_search.py, written from the reference's `band.rs` and `lib.rs` and
from DESIGN.md, sharing nothing with `csrc/band_search.hpp`.

* Start (`band.rs:13-23`, `lib.rs:131-143`): `(start_f, start_inc)` is `(0, 1)` for start `zero`, `(gap, gap)` for `gap` (the unit gap
  cost `|n - m|` between the corners) and `(h0, 1)` for `h0`.  Linear search tries `start_f` first.  Band doubling has
  `offset = start_f` and tries `offset + max(start_inc, block_width)` first.
* One round (`band.rs:115-140`, `157-181`): `f(s)` is `None` or `Some(cost)`.  `Some(cost)` with `cost <= s` ends the search.  Any other
  `Some(cost)` is an upper bound: `maxs = min(maxs, cost)`.  Then `last_s = s` and `s = min(next(s), maxs)`, where `next(s)` is
  `s + delta` for linear search and `max(ceil(factor * (s - offset) as f32), 1) + offset` for band doubling; the product is
  float32 arithmetic (numpy.float32 here).
* The reference's three `assert!`s do not abort here but are counted: `cost > maxs`; `cost <= last_s` on the
  successful pass; `None` after some pass already gave an upper bound.
* Never stall: when `min(next(s), maxs)` would not exceed `s` -- the pass at `s == maxs` did not succeed -- the next
  bound is `next(s)` without the cap.

`search` returns what it tried and saw, so that the test can assert that its scripts reached every corner."""
import math
from fractions import Fraction

import numpy as np

COST_MAX = 2**31 - 1


def search(doubling, start, factor, delta, h0, gap, block_width, f):
    """doubling 'band' | 'linear'; start 'zero' | 'gap' | 'h0'; f(s) -> None | cost.
    -> dict(bounds=[s, ...], cost, sanity, events=set of names)."""
    start_f, start_inc = {"zero": (0, 1), "gap": (gap, gap), "h0": (h0, 1)}[start]
    events = set()
    if doubling == "linear":
        offset, s = None, start_f
    else:
        offset = start_f
        events.add("block_width_above_start_inc" if block_width > start_inc else "block_width_below_start_inc" if block_width < start_inc else "block_width_is_start_inc")
        s = offset + max(start_inc, block_width)

    def nxt(x):
        if doubling == "linear":
            return x + delta
        prod = np.float32(factor) * np.float32(x - offset)
        assert prod.dtype == np.float32
        grown = int(np.ceil(prod))
        if x - offset > 2**24 and grown != math.ceil(Fraction(factor) * (x - offset)):  # (what exact arithmetic would give)
            events.add("f32_inexact")
        return max(grown, 1) + offset

    last_s, maxs, sanity, bounds = -1, COST_MAX, 0, []
    while True:
        bounds.append(s)
        cost = f(s)
        if cost is not None:
            if cost > maxs:
                sanity += 1
                events.add("sanity_cost_above_maxs")
            if cost <= s:
                if cost <= last_s:
                    sanity += 1
                    events.add("sanity_cost_within_last_s")
                return dict(bounds=bounds, cost=cost, sanity=sanity, events=events)
            maxs = min(maxs, cost)
        elif maxs != COST_MAX:
            sanity += 1
            events.add("sanity_none_after_bound")
        last_s = s
        s = nxt(last_s)
        if maxs < s:
            s = maxs
            events.add("capped_by_maxs")
        if s <= last_s:
            s = nxt(last_s)
            events.add("never_stall")
