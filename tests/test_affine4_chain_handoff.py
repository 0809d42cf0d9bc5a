"""The hand-off of a 16-byte boundary value of the chained double-affine route as two 8-byte halves (csrc/affine4_chain_value.hpp),
without a GPU: tests/affine4_chain_handoff.cpp, a stand-alone program with its own main, runs one producer and one consumer thread over
a row preset to all-ones, the halves written in both orders, and checks that every accepted column is the triple that was written
(M = 2^30, I = 2^30 + 2000 and I2 = 0 included) and that a half-written column is never accepted.  Built under ThreadSanitizer where the
toolchain has it (as tests/test_rdv_emu.py's program is), else without; the program's own checks hold either way."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "astar-pairwise-aligner_amd" / "csrc"


def test_two_halves_between_two_threads(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    assert "#include <hip" not in (CSRC / "affine4_chain_value.hpp").read_text()  # plain C++: the system compiler builds it below
    exe = tmp_path / "affine4_chain_handoff"
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", str(CSRC), str(ROOT / "tests" / "affine4_chain_handoff.cpp"),
            "-o", str(exe)]
    tsan = subprocess.run(base + ["-fsanitize=thread"], capture_output=True, text=True)
    if tsan.returncode != 0:  # a toolchain without ThreadSanitizer: the same program, without the race detector
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
    word, cols, rounds, _halves = r.stdout.split()
    assert word == "ok" and int(cols) >= 2000 and int(rounds) == 4


def test_the_kernel_uses_the_same_packing():
    """The kernel header includes the plain header and takes pack() and delivered() from it, and stores and loads 8-byte halves."""
    k = (CSRC / "affine4_chain_kernel.hpp").read_text()
    assert '#include "affine4_chain_value.hpp"' in k
    assert "affine4_chain::delivered(" in k and "affine4_chain::pack(" in k
    v = (CSRC / "affine4_chain_value.hpp").read_text()
    assert "static_assert(kLayerMax < 0xFFFFFFFFu" in v
