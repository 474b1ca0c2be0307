"""Block solves on small generators with and without option block_small ("Small generators").  Writes
profiles/block_small.json and prints it as ONE JSON line:

  - kfsp_expv_block (t = 0.1, tol = 1e-8, m = 30, the figures profiles/block_spmm.py uses for c2) on the golden toggle FSP
    (SELL) and on synth.toggle(60, 50) stored as SELL and as banded, k = 1, 2, 4, 8, 16 start columns (probability bumps);
  - block_small = 0 and 1 alternating in one process on one context, median of 5 solves each after a warm-up of both:
    wall ms per solve and per step, the phase timers per step (begin, arnoldi, combine, host Pade) and kfsp_block_info;
  - the single-vector pass on the same generator (kfsp_begin_step + kfsp_arnoldi(30, 1, 2), one launch of k_arnoldi_small)
    as wall ms per pass, median of 50: the figure the block pass is to be read against.

    python profiles/block_small.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from krylovfspssa_amd import KfspContext, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 4, 8, 16)
T, TOL, M = 0.1, 1e-8, 30
PHASES = ("begin_step", "arnoldi", "combine", "host_pade")


def golden_toggle(ctx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "assembly_toggle_k20.npz"))
    ctx.set_option("format", 1)
    ctx.set_option("sell_code", 0)
    ctx.set_matrix_ell(g["adj"], g["offdiag"], g["diag"])


def toggle_sell(ctx):
    ctx.set_option("format", 1)
    ctx.set_option("sell_code", 0)
    ctx.set_matrix_ell(*synth.toggle(60, 50).ell())


def toggle_banded(ctx):
    mdl = synth.toggle(60, 50)
    ctx.set_option("format", 0)
    ctx.set_option("dia_mask", 0)
    ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())


def start_columns(n, rng):
    """16 probability columns: smooth bumps of different widths around different states"""
    W = np.zeros((n, 16))
    x = np.arange(n)
    for c in range(16):
        p = np.exp(-0.5 * ((x - (n * (c + 1)) // 18) / (3.0 + 2.0 * c)) ** 2) + 1e-3 * rng.random(n)
        W[:, c] = p / p.sum()
    return W


def solve(ctx, W, small):
    ctx.set_option("block_small", small)
    ctx.set_block(W)
    ctx.timers(reset=True)
    t0 = time.perf_counter()
    ws, st = ctx.expv_block(T, TOL, M)
    wall = (time.perf_counter() - t0) * 1e3
    tm = ctx.timers()
    passes = st.nstep                                          # one begin / arnoldi / combine per step
    rec = {"wall_ms": wall, "ms_per_step": wall / passes, "nstep": st.nstep, "nreject": st.nreject}
    for p in PHASES:
        rec[p + "_ms_per_step"] = tm[p] / passes
    return rec, ctx.block_info(), float(ws.min())


def median_of(recs):
    return {key: (round(float(np.median([r[key] for r in recs])), 5) if isinstance(recs[0][key], float) else recs[0][key])
            for key in recs[0]}


def single_pass_ms(ctx, w, reps=50):
    ctx.set_vector(w)
    out = []
    for _ in range(reps + 5):
        t0 = time.perf_counter()
        ctx.begin_step()
        t1 = time.perf_counter()
        ctx.arnoldi(M, 1, 2, 1e-7)
        out.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    out = np.array(out[5:])
    return {"begin_step_ms": round(float(np.median(out[:, 0])), 5), "arnoldi_ms": round(float(np.median(out[:, 1])), 5),
            "arnoldi_us_per_column": round(float(np.median(out[:, 1])) * 1e3 / (M + 1), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_small.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res = {"what": "kfsp_expv_block with block_small = 0 / 1, alternating, median of 5", "t": T, "tol": TOL, "m": M, "generators": {}}
    for name, setter in (("golden_toggle_sell", golden_toggle), ("toggle_60x50_sell", toggle_sell), ("toggle_60x50_banded", toggle_banded)):
        with KfspContext(0) as ctx:
            setter(ctx)
            W = start_columns(ctx.n, rng)
            gen = {"n": ctx.n, "format": ctx.layout_info()["format"], "single_vector_pass": single_pass_ms(ctx, W[:, 0]), "k": {}}
            for k in KS:
                for small in (0, 1):
                    solve(ctx, W[:, :k], small)                # warm-up: allocations, code objects, LDS attribute
                runs = {0: [], 1: []}
                info = {}
                mass = {}
                for _ in range(5):
                    for small in (0, 1):
                        rec, info[small], mass[small] = solve(ctx, W[:, :k], small)
                        runs[small].append(rec)
                off, on = median_of(runs[0]), median_of(runs[1])
                gen["k"][str(k)] = {"block_small_0": off, "block_small_1": on, "info_0": info[0], "info_1": info[1],
                                    "wall_ratio_1_over_0": round(on["wall_ms"] / off["wall_ms"], 3),
                                    "min_mass": [mass[0], mass[1]]}
            res["generators"][name] = gen
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
