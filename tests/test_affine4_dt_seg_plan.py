"""The host geometry of the segmented traceback of the double-affine diagonal-transition route (csrc/affine4_dt_seg_plan.hpp), without a
GPU: tests/affine4_dt_seg_plan_driver.cpp, a stand-alone program, is built with the system C++ compiler under the address and
undefined-behaviour sanitizers and run as a child process.  Over 300 seeded batches like those of tests/test_affine4_dt_plan.py (the four
ends settings; s_max 0, small, a few thousand and 2^30 - 1; seg Ew, Ew + 1, a few Ew, 2^30 - 1 and the default; budgets from one chunk down
to the largest pair alone and a few bytes below it) under the three models of the tests, STEEP (Ew = 9 above E = 2) and one with costs of
1000 it checks: E, Ew, H, S and nseg as the header states them; every read s - c of the recurrence and of the walk, for s in a segment,
lands through the kernels' row arithmetic on the row of that very front in that ring's head or body (the kNeg row where s < c); the
checkpoint rows of the forward pass are within the pair's checkpoint rows, distinct, and those the fill copies to the ring's head; the
four regions of a pair are 4-byte aligned, disjoint and inside the chunk; every chunk is within the budget and full; the refused pair is
the first over budget; the byte formula; and the pinned 36 ring rows and H = 30 under double_affine(4, 6, 2, 24, 1)."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "astar-pairwise-aligner_amd" / "csrc"


def test_seg_plan_properties_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "affine4_dt_seg_plan_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(ROOT / "tests" / "affine4_dt_seg_plan_driver.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    word, batches, chunks, reads, checkpoints = r.stdout.split()
    assert word == "ok" and int(batches) == 300
    assert int(chunks) >= 250  # (a quarter of the batches is refused)
    assert int(reads) >= 100_000 and int(checkpoints) >= 100_000
