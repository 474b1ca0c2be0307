"""What option block_integral costs ("Time integrals").  Writes profiles/block_integral.json and prints it
as ONE JSON line.  On the toggle box of config 2 (synth.toggle(1000, 1000), 10^6 states, stored banded), k = 4 and 16, m = 30:

  - the combine alone: after kfsp_block_begin + kfsp_block_arnoldi(30), kfsp_block_combine(32, ...) with the option off
    (k_bcombine, the parent's behaviour) and on (k_bcombine_int), alternating, median of 20 calls each after a warm-up:
    wall ms per call (one table upload, the combine launch, the one-workgroup sum launch, 128 bytes back, one
    synchronisation) and the bytes the layout says each kernel moves, hence GB/s;
  - whole solves: kfsp_expv_block(t = 0.1, tol = 1e-8, m = 30) with the option 0 and 1, alternating, median of 5: wall ms,
    steps, and the phase timers per step (combine, host Pade - the extra Pade of the option lands there).

For per-kernel device times run it once, on its own, under a kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/block_integral.py --quick

    python profiles/block_integral.py [--out FILE] [--quick]
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
T, TOL, M = 0.1, 1e-8, 30
PHASES = ("begin_step", "arnoldi", "combine", "host_pade")


def kp_of(k):
    return 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16


def combine_calls(ctx, W, reps):
    k = W.shape[1]
    mx = M + 2
    rng = np.random.default_rng(1)
    coef = rng.standard_normal((mx, k)) * 1e-3
    cj = rng.standard_normal((mx, k)) * 1e-6
    ms = {0: [], 1: []}
    for opt in (0, 1):                                        # a block (and J) per setting, one basis each
        ctx.set_option("block_integral", opt)
        ctx.set_block(W)
        ctx.block_begin(M)
        ctx.block_arnoldi(M)
        for r in range(reps + 3):
            t0 = time.perf_counter()
            ctx.block_combine(mx, coef, coef_integral=cj if opt else None)
            if r >= 3:
                ms[opt].append((time.perf_counter() - t0) * 1e3)
    rows = ((ctx.n + 127) // 128) * 128
    col = rows * kp_of(k) * 8
    out = {}
    for opt in (0, 1):
        moved = (mx + 1 + 2 * opt) * col                      # the basis once, W written; J read and written
        med = float(np.median(ms[opt]))
        out[f"block_integral_{opt}"] = {"ms_per_call": round(med, 4), "min_ms": round(min(ms[opt]), 4), "bytes": moved,
                                        "GBps": round(moved / med * 1e-6, 1)}
    out["ratio_1_over_0"] = round(out["block_integral_1"]["ms_per_call"] / out["block_integral_0"]["ms_per_call"], 4)
    out["ratio_of_bytes"] = round((mx + 3) / (mx + 1), 4)
    ctx.set_option("block_integral", 0)
    return out


def solve(ctx, W, opt):
    ctx.set_option("block_integral", opt)
    ctx.set_block(W)
    ctx.timers(reset=True)
    t0 = time.perf_counter()
    ws, st = ctx.expv_block(T, TOL, M)
    wall = (time.perf_counter() - t0) * 1e3
    tm = ctx.timers()
    rec = {"wall_ms": wall, "nstep": st.nstep, "nreject": st.nreject}
    for p in PHASES:
        rec[p + "_ms_per_step"] = tm[p] / st.nstep
    return rec


def median_of(recs):
    return {key: (round(float(np.median([r[key] for r in recs])), 5) if isinstance(recs[0][key], float) else recs[0][key])
            for key in recs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_integral.json"))
    ap.add_argument("--quick", action="store_true", help="3 combine calls and 1 solve per setting (for a kernel trace)")
    args = ap.parse_args()
    reps_c, reps_s = (3, 1) if args.quick else (20, 5)
    mdl = synth.toggle(1000, 1000)
    W = np.zeros((mdl.n, 16))
    for j in range(16):
        W[:, j] = synth.poisson_p0(mdl, 5.0 + 10.0 * j)
    res = {"what": "option block_integral 0 / 1 on toggle(1000, 1000) stored banded, m = 30", "t": T, "tol": TOL, "m": M, "k": {}}
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(mdl, store=True)
        res["n"], res["format"] = ctx.n, ctx.layout_info()["format"]
        for k in (4, 16):
            rec = {"combine": combine_calls(ctx, W[:, :k], reps_c)}
            for opt in (0, 1):
                solve(ctx, W[:, :k], opt)                      # warm-up
            runs = {0: [], 1: []}
            for _ in range(reps_s):
                for opt in (0, 1):
                    runs[opt].append(solve(ctx, W[:, :k], opt))
            off, on = median_of(runs[0]), median_of(runs[1])
            rec["solve"] = {"block_integral_0": off, "block_integral_1": on,
                            "wall_ratio_1_over_0": round(on["wall_ms"] / off["wall_ms"], 4)}
            res["k"][str(k)] = rec
    if not args.quick:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
