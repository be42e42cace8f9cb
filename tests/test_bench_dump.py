"""bench.py --dump-outputs: what the timed path returned, written as float32 .npy files within 64 MB (a fixed, seeded sample
beyond that).  CPU tests of the writer; the GPU version, with the real bench.py, is
tests/test_gpu_multi.py::test_bench_dump_outputs_are_the_planes_of_the_last_step."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_output_is_written_whole_as_float32(tmp_path):
    bench = _bench()
    a = (np.arange(2 * 30 * 50) % 256).astype(np.uint8).reshape(2, 30, 50)
    rec = bench.dump_outputs(tmp_path, {"output": a})
    got = np.load(tmp_path / "output.npy")
    assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a)
    assert rec["output"]["shape"] == [2, 30, 50] and "sample" not in rec["output"]


def test_large_output_is_a_fixed_sample_within_the_budget(tmp_path):
    bench = _bench()
    a = np.arange(100_000, dtype=np.int32)                 # value == flat index: the sample shows which elements it took
    budget = 64 << 10
    bench.dump_outputs(tmp_path / "a", {"output": a}, budget=budget)
    bench.dump_outputs(tmp_path / "b", {"output": a}, budget=budget)
    s = np.load(tmp_path / "a" / "output.npy")
    assert (tmp_path / "a" / "output.npy").stat().st_size <= budget and s.dtype == np.float32
    assert np.array_equal(s, np.load(tmp_path / "b" / "output.npy"))             # the same elements in every run
    block = -(-a.size // ((budget - 4096) // 4))
    assert s.size == a.size // block and np.array_equal(s.astype(np.int64) // block, np.arange(s.size))   # one per block


def test_default_budget_holds_for_the_largest_single_gpu_output(tmp_path):
    """--path pipeline at the default size returns 3840x2160x3 bytes: 99.5 MB as float32, so it is sampled to within 64 MB."""
    bench = _bench()
    a = np.zeros((1, 2160, 3840, 3), np.uint8)
    rec = bench.dump_outputs(tmp_path, {"output": a})
    assert "sample" in rec["output"] and (tmp_path / "output.npy").stat().st_size <= 64 << 20


def test_steps_below_one_are_refused():
    """ms_per_step is the timed window over --steps: zero steps is not a measurement (refused before any GPU call)."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr[-500:]
