"""Every Python script of the repository parses (bench.py and the measurement tools only run on the GPU box: a syntax slip there would
otherwise show up at the end of a round)."""
import glob
import os
import py_compile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = sorted(glob.glob(os.path.join(ROOT, "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) +
                 glob.glob(os.path.join(ROOT, "tests", "tools", "*.py")) + glob.glob(os.path.join(ROOT, "astar-pairwise-aligner_amd", "*.py")))


@pytest.mark.parametrize("path", SCRIPTS, ids=[os.path.relpath(p, ROOT) for p in SCRIPTS])
def test_script_compiles(path, tmp_path):
    py_compile.compile(path, cfile=str(tmp_path / "x.pyc"), doraise=True)


def test_bench_flags_without_a_gpu():
    """bench.py --help works on a box without a GPU (argument parsing comes before any device work)."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--gpus" in out.stdout and "--steps" in out.stdout and "--warmup" in out.stdout


def test_bench_dump_outputs_without_a_gpu(tmp_path):
    """bench.py offers --full and --dump-outputs; its dump writes float64 .npy files, all of a batch up to the cap and a fixed seeded
    sample (with the indices) beyond it -- the same sample from run to run.  (In a child process: importing bench.py sets HIP variables.)"""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
    code = (
        "import importlib.util, sys, numpy as np\n"
        f"spec = importlib.util.spec_from_file_location('bench', {os.path.join(ROOT, 'bench.py')!r})\n"
        "b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)\n"
        "d = sys.argv[1]\n"
        "b.dump_costs(d + '/small', np.arange(100, dtype=np.int32))\n"
        "big = np.arange(b.DUMP_MAX_VALUES + 1000, dtype=np.int32) * 3\n"
        "b.dump_costs(d + '/big1', big)\n"
        "b.dump_costs(d + '/big2', big)\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    import numpy as np

    small = np.load(tmp_path / "small" / "costs.npy")
    assert small.dtype == np.float64 and small.tolist() == list(range(100)) and not (tmp_path / "small" / "costs_index.npy").exists()
    v1, i1 = np.load(tmp_path / "big1" / "costs.npy"), np.load(tmp_path / "big1" / "costs_index.npy")
    v2, i2 = np.load(tmp_path / "big2" / "costs.npy"), np.load(tmp_path / "big2" / "costs_index.npy")
    assert v1.dtype == i1.dtype == np.float64 and len(v1) == len(i1) < 2_200_000
    assert np.array_equal(v1, v2) and np.array_equal(i1, i2) and np.array_equal(v1, i1 * 3)
    assert v1.nbytes + i1.nbytes <= 64 * 10**6
