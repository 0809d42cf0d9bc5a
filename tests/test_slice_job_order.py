"""The ticket order of the bit-sliced kernel's (group, strip) jobs (csrc/slice_job_order.hpp), without a GPU:
tests/slice_job_order_driver.cpp, a stand-alone program, is built with the system C++ compiler under the address and undefined-behaviour
sanitizers and run as a child process.  Over 400 seeded random plans (1 .. 300 groups of 1 .. 40 strips, 1 .. 4096 wave slots, chain
lengths 0, 1, 2, 3, 8 and the automatic one) it checks that the list is a permutation of all (group, strip), that every strip's
producer holds a lower ticket, that within a band a group's strips are contiguous and ascending, that chain 0 and any chain >= the
longest group give the group-major order and chain 1 the strip-major one, and the automatic chain length of the two headline shapes."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "astar-pairwise-aligner_amd" / "csrc"


def test_job_order_properties_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "slice_job_order_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(ROOT / "tests" / "slice_job_order_driver.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    word, plans = r.stdout.split()
    assert word == "ok" and int(plans) == 400
