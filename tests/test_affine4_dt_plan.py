"""The host geometry of the double-affine diagonal-transition route (csrc/affine4_dt_plan.hpp), without a GPU:
tests/affine4_dt_plan_driver.cpp, a stand-alone program, is built with the system C++ compiler under the address and undefined-behaviour
sanitizers and run as a child process.  Over 320 seeded batches (|a| and |b| in 0 .. 300, some up to 3000, empty sequences among them;
s_max 0, small, a few thousand and 2^30 - 1; cost-only and traced; the four ends settings; budgets from one chunk down to the largest pair
alone and a few bytes below it) under the three models of the tests and one with costs of 1000 it checks: the five ring depths as
DESIGN.md states them; every read s - c of the recurrence, through the kernel's slot arithmetic, finds the front it asks for; kmin, kmax
and W hold the live range of every cost up to the bound and are tight; the pairs' buffers are 4-byte aligned, disjoint and inside their
chunk; every chunk is within the budget and full; the refused pair is the first over budget; and the pinned sizes, 36 rows of W values
per pair under double_affine(4, 6, 2, 24, 1)."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "astar-pairwise-aligner_amd" / "csrc"


def test_plan_properties_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "affine4_dt_plan_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(ROOT / "tests" / "affine4_dt_plan_driver.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    word, batches, chunks, reads = r.stdout.split()
    assert word == "ok" and int(batches) == 320
    assert int(chunks) >= 250  # (a fifth of the batches is refused)
    assert int(reads) >= 100_000
