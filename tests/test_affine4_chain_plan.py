"""The host-side planner of the chained routes (csrc/affine_chain_plan.hpp) with the 16-byte boundary values of the double-affine
batch, without a GPU: tests/affine4_chain_plan_driver.cpp, a stand-alone program, is built with the system C++ compiler under the
address and undefined-behaviour sanitizers and run as a child process.  Over 400 seeded random batches (|b| in 1025 .. 40 000, |a| in
0 .. 5000, budgets from one chunk to a refusal) it checks, with value_bytes = 16, that every job's producer is the job before it, that
a pair's jobs are contiguous and ascending, that the boundary rows of a chunk neither overlap nor leave its allocation, that every chunk
is within the budget in bytes, that exactly the pairs over budget are refused, and that the job count is the sum of ceil(|b| / 1024);
and that plan(pairs, B) is plan(pairs, B, 8)."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "astar-pairwise-aligner_amd" / "csrc"


def test_planner_properties_with_16_byte_values_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "affine4_chain_plan_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(ROOT / "tests" / "affine4_chain_plan_driver.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    word, batches, refused = r.stdout.split()
    assert word == "ok" and int(batches) == 400
    assert 50 <= int(refused) <= 100  # every fourth batch asks for a budget below its biggest pair
