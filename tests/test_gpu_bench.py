"""bench.py on the device through a one-rank RCCL communicator (--force-comm): the JSON contract, and
what happens when the distributed product RAISES on some rank (here: injected) - the communicator is
thrown away and made anew, the next simpler exchange is tried, and only if every mode raises does the
job stop with exit code 3 instead of printing a number."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(extra_env, *flags):
    env = dict(os.environ, **extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--force-comm",
                           "--no-cpu", "--no-expv", "--steps", "5", "--warmup", "2", *flags],
                          cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_bench_line_through_a_one_rank_communicator():
    r = _bench({})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1                                         # exactly one JSON line on stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["steps"] == 5 and j["warmup"] == 2 and j["unit"] == "GB/s"
    assert j["self_check"]["ok"] and j["config"]["exchange"].startswith("halo strips (banded generator)")
    assert set(j["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "frac_traffic", "alg_GBps"}
    assert 0.0 < j["roofline"]["frac"] <= 1.0                      # bytes that really move / peak: never above 1


def test_a_raising_product_recreates_the_communicator_and_steps_down():
    r = _bench({"KFSP_BENCH_INJECT_RAISE": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["self_check"]["ok"] and "not overlapped" in j["config"]["exchange"]
    assert "product failed on some rank" in r.stderr
    r = _bench({"KFSP_BENCH_INJECT_RAISE": "1,2"})
    assert r.returncode == 0
    assert "all-gather of the whole vector" in json.loads(r.stdout.strip().splitlines()[-1])["config"]["exchange"]


def test_a_product_that_raises_in_every_mode_stops_the_job():
    r = _bench({"KFSP_BENCH_INJECT_RAISE": "1,2,3"})
    assert r.returncode == 3 and not r.stdout.strip()
    assert "raised in every exchange mode" in r.stderr


def _plain(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny",
                           "--steps", "5", "--warmup", "2", *flags],
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_a_plain_run_dumps_the_timed_product_and_measures_nothing_else(tmp_path):
    """the plain line: the headline and its roofline, none of the --full blocks; --dump-outputs writes y = A x of the
    seeded input, equal to numpy's product and bit for bit the same on a second run"""
    import numpy as np
    from bench import spmv_model
    ys = []
    for d in ("a", "b"):
        r = _plain("--dump-outputs", str(tmp_path / d))
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["steps"] == 5 and j["ms_per_step"] > 0 and j["dtype"] == "f64" and j["unit"] == "GB/s"
        assert not set(j) & {"self_check", "matrix_free", "spmv_1e7", "expv", "expv_workload", "cpu_baseline"}
        assert j["exchange"] is None and "roofline" in j
        ys.append(np.load(tmp_path / d / "y.npy"))
    y = ys[0]
    assert y.dtype == np.float64 and np.array_equal(y, ys[1])
    mdl, _ = spmv_model("tiny", 1)
    rp, cc, vv = mdl.csr_rows(0, mdl.n)
    x = np.random.default_rng(12345).random(mdl.n)               # bench.py's input of rank 0
    assert len(y) == mdl.n == j["config"]["states_per_gpu"]
    ref = np.add.reduceat(vv * x[cc], rp[:-1])
    mag = np.add.reduceat(np.abs(vv) * x[cc], rp[:-1])
    assert np.max(np.abs(y - ref) / (mag + 1e-300)) < 1e-12


def test_full_adds_the_checks_and_the_other_measurements():
    r = _plain("--full")
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["self_check"]["ok"] and j["matrix_free"]["self_check"]["ok"]
    assert j["expv"]["ms_per_step"] > 0 and j["expv"]["l1_err_vs_cpu"] < 1e-10
    assert j["cpu_baseline"]["value"] > 0
