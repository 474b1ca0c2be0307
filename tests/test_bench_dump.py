"""bench.py --dump-outputs on the host: an output within the budget is written whole, a larger one as
the same seeded sample on every call, never above the budget; a plain command line leaves --full off.
(CPU only: the arrays here are numpy, not products of the device.)"""
import os
import sys

import numpy as np

from tests.conftest import ROOT

sys.path.insert(0, ROOT)


def test_an_output_within_the_budget_is_written_whole(tmp_path):
    import bench
    y = np.random.default_rng(0).random(1000)
    p = bench.dump_output(str(tmp_path / "out"), "y", y, 1 << 20)
    assert p == str(tmp_path / "out" / "y.npy")
    z = np.load(p)
    assert z.dtype == np.float64 and np.array_equal(z, y)


def test_a_larger_output_is_the_same_seeded_sample_on_every_run(tmp_path):
    import bench
    y = np.arange(100_000, dtype=np.float64)
    budget = 4096 + 8 * 5000
    a = np.load(bench.dump_output(str(tmp_path / "a"), "y", y, budget))
    b = np.load(bench.dump_output(str(tmp_path / "b"), "y", y.copy(), budget))
    assert a.dtype == np.float64 and len(a) == 5000 and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0)                           # distinct entries, in index order
    assert os.path.getsize(tmp_path / "a" / "y.npy") <= budget


def test_a_plain_command_line_leaves_full_off(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
