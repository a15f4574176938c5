"""bench.py's command line and its --dump-outputs writer, without a GPU."""

import ast
import os
import subprocess
import sys

import numpy as np

from helpers import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _dump_outputs():
    """bench.dump_outputs and its budget, compiled from the source (importing bench.py would pin CPUs and load torch)."""
    tree = ast.parse(open(BENCH).read())
    keep = [n for n in tree.body
            if (isinstance(n, ast.FunctionDef) and n.name == "dump_outputs")
            or (isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "DUMP_BUDGET_BYTES" for t in n.targets))]
    assert len(keep) == 2
    ns = {"os": os, "np": np}
    exec(compile(ast.Module(keep, []), "bench.py", "exec"), ns)
    return ns["dump_outputs"], ns["DUMP_BUDGET_BYTES"]


def test_dump_outputs_writes_float32_within_the_budget(tmp_path):
    dump, budget = _dump_outputs()
    assert budget <= 64_000_000
    rng = np.random.Generator(np.random.PCG64(3))
    small = rng.integers(0, 256, size=(1080, 1920, 4), dtype=np.uint8)      # psp presets: written whole
    dump(str(tmp_path / "a"), {"output": small})
    got = np.load(tmp_path / "a" / "output.npy")
    assert got.dtype == np.float32 and got.shape == small.shape and np.array_equal(got, small)
    large = rng.integers(0, 256, size=(1792, 2560, 4), dtype=np.uint8)      # ps2-quality: a fixed sample
    for d in ("b", "c"):
        dump(str(tmp_path / d), {"output": large})
    b, c = np.load(tmp_path / "b" / "output.npy"), np.load(tmp_path / "c" / "output.npy")
    assert b.dtype == np.float32 and b.ndim == 1 and 0.5 * budget < b.nbytes <= budget - 4096
    assert np.array_equal(b, c)                                              # the same elements every run
    assert os.path.getsize(tmp_path / "b" / "output.npy") <= budget


def test_bench_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout and "--steps" in r.stdout
