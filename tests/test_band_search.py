"""The schedule of A*PA2's outer loop (csrc/band_search.hpp: start bound, next bound, upper-bound cap, the three counted sanity events
and the never-stall rule), without a GPU: tests/band_search_driver.cpp, a stand-alone program, is built with the system C++ compiler
under the address and undefined-behaviour sanitizers and run as a child process over 432 seeded scripted searches.  Every script's
sequence of bounds, result and sanity count is compared exactly with tests/band_search_plain.py, a plain loop written from the
reference's band.rs / lib.rs and DESIGN.md with numpy.float32 for the f32 product.

The grid: band doubling with factor 1.5 and 2.0, linear search with delta 1 and 300; start zero / gap / h0; gap 0, 300 and 20 000 001
(above 2^24: the f32 product is inexact from the first step); block width 1, 64, 256; four seeds each.  The outcome of each pass is
drawn while the plain loop runs, so that it can depend on the bound: None, Some(above the bound) -- an upper bound that caps what
follows --, Some(above that upper bound), Some(within the bound), Some(within the previous bound).  The test asserts that every one
of these corners was reached, not that the generator was meant to reach it."""
import random
import shutil
import subprocess
from pathlib import Path

from tests import band_search_plain as plain

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "astar-pairwise-aligner_amd" / "csrc"

SCHEDULES = [("band", 1.5, 0), ("band", 2.0, 0), ("linear", 0.0, 1), ("linear", 0.0, 300)]
STARTS = ["zero", "gap", "h0"]
GAPS = [0, 300, 20_000_001]
WIDTHS = [1, 64, 256]
SEEDS = 4
MAX_PASSES = 12        # then the script lets the search succeed
MAX_BOUND = 1 << 29    # likewise: the bounds stay inside int32


def scripted(rng):
    """f(s) for the plain loop; remembers what it answered."""
    outcomes, upper = [], []

    def f(s):
        roll = rng.random()
        if len(outcomes) >= MAX_PASSES or s > MAX_BOUND:
            cost = rng.randint(0, s)             # found, perhaps within an earlier bound
        elif roll < 0.45:
            cost = None
        elif roll < 0.70:
            cost = s + rng.randint(1, 1000)      # an upper bound
        elif roll < 0.80 and upper:
            cost = min(upper) + rng.randint(1, 10)
        elif roll < 0.90:
            cost = rng.randint(max(0, s - 3), s)  # found
        else:
            cost = rng.randint(0, s)
        if cost is not None and cost > s:
            upper.append(cost)
        outcomes.append(cost)
        return cost

    return f, outcomes


def test_scripted_searches_match_the_plain_loop_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "band_search_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(ROOT / "tests" / "band_search_driver.cpp"), "-o", str(exe)], check=True)
    lines, want, seen = [], [], {}
    for doubling, factor, delta in SCHEDULES:
        for start in STARTS:
            for gap in GAPS:
                for width in WIDTHS:
                    for seed in range(SEEDS):
                        rng = random.Random(f"{doubling} {factor} {delta} {start} {gap} {width} {seed}")
                        h0 = rng.randint(0, 500)
                        f, outcomes = scripted(rng)
                        r = plain.search(doubling, start, factor, delta, h0, gap, width, f)
                        for e in r["events"]:
                            seen.setdefault(e, set()).add((doubling, factor, delta, start, gap, width))
                        script = [-1 if c is None else c for c in outcomes]
                        lines.append(" ".join(map(str, [1 if doubling == "band" else 2, STARTS.index(start), factor, delta, h0, gap, width, len(script)] + script)))
                        want.append(" ".join(map(str, [len(r["bounds"])] + r["bounds"] + [1, r["cost"], r["bounds"][-1], r["sanity"]])))
    assert len(lines) == 432
    # every corner occurred
    for e in ("sanity_cost_above_maxs", "sanity_cost_within_last_s", "sanity_none_after_bound", "capped_by_maxs", "never_stall", "f32_inexact",
              "block_width_above_start_inc", "block_width_below_start_inc"):
        assert seen.get(e), e
    for e in ("capped_by_maxs", "never_stall"):  # under band doubling and under linear search
        assert {c[0] for c in seen[e]} == {"band", "linear"}, e
    assert {c[1] for c in seen["f32_inexact"]} == {1.5, 2.0}
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (lines[i], g, w)
