"""Transposed block product on dictionary-coded banded generators (option block_dia_code_adjoint, k_spmm_diac_t; DESIGN.md
12, "Coded banded generators, backward").  Writes ONE JSON object (--out, default profiles/block_dia_code_adjoint.json) and
prints it.

Steps, each in a child process of its own under its own time limit (the parent never opens the device; a step that fails or
runs out of time ends the run there):

  c3, c3x   the repressilator box 171^3 (5.0e6 states) and 216^3 (1.0e7), stored as diagonals on the device, dia_code at its
            default (both lie beyond the Infinity Cache: the coded image builds itself).  For k = 1, 2, 4, 8, 16, in ONE
            process and on one resident block, with adjoint = 1 and block_dia_code = 1 throughout: kfsp_spmm_bench with
            block_dia_code_adjoint alternating 0, 1, 0, 1, ... - HIP-event windows of --reps launches, --windows windows
            per setting, median and spread (max - min) of each.  The plain transposed block (k_spmm_t) of the same process
            is the baseline of every ratio.  A width counts as a gain only where the coded median lies below the plain one
            by more than THREE times the larger of the two spreads.
  solve     the backward kfsp_expv_block on c2 (toggle 1000 x 1000, dia_code = 1) at k = 8, m = 30, the two settings
            alternating; wall time, steps, and whether W came out bit-identical.

    python profiles/block_dia_code_adjoint.py [--steps c3,c3x,solve] [--ks 1,2,4,8,16] [--reps 200] [--windows 5] [--limit 420]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

GENERATORS = {"c3": (171, 171, 171), "c3x": (216, 216, 216)}
HBM_BYTES_PER_S = 8.0e12
OPT = "block_dia_code_adjoint"


def kp_of(k):
    return 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16


def summary(ms):
    return {"ms": round(statistics.median(ms), 5), "spread_ms": round(max(ms) - min(ms), 5), "windows_ms": [round(t, 5) for t in ms]}


def step_products(name, ks, reps, windows):
    import numpy as np
    from krylovfspssa_amd import KfspContext, synth
    mdl = synth.repressilator(dims=GENERATORS[name])
    X = np.random.default_rng(0).random((mdl.n, max(ks)))
    out = {"n": mdl.n, "dims": list(mdl.dims)}
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(mdl, store=True)               # dia_code stays at its default -1
        lay, ci = ctx.layout_info(), ctx.dia_code_info()
        rows, nd, rec = lay["chunks"] * 64, ci["diagonals"], ci["record_bytes"]
        out.update(format=lay["format"], rows=rows, diagonals=nd,
                   code={key: ci[key] for key in ("active", "width", "record_bytes", "dict_bytes", "diag_table_bytes")})
        assert ci["active"] == 1, ci
        ctx.set_option("block_dia_code", 1)
        ctx.set_option("adjoint", 1)
        out["spmm_t"] = {}
        for k in ks:
            kp = kp_of(k)
            ctx.set_block(X[:, :k])
            ms = {0: [], 1: []}
            for opt in (0, 1):
                ctx.set_option(OPT, opt)
                ctx.spmm_bench(5)
            for _ in range(windows):
                for opt in (0, 1):
                    ctx.set_option(OPT, opt)
                    ms[opt].append(ctx.spmm_bench(reps) / reps)
                    info = ctx.block_info()
                    assert info["adjoint"] == 1 and info["fmt"] == (9 if opt else 0), info
            plain, coded = summary(ms[0]), summary(ms[1])
            bytes_row = {"plain": 8 * nd + 8 + 16 * kp, "coded": rec + 8 + 16 * kp}
            for s, key in ((plain, "plain"), (coded, "coded")):
                s["ms_per_vector"] = round(s["ms"] / k, 5)
                s["layout_bytes_per_row"] = bytes_row[key]
                s["fraction_of_8TBps"] = round(bytes_row[key] * rows / (s["ms"] * 1e-3) / HBM_BYTES_PER_S, 3)
            out["spmm_t"][str(k)] = {
                "kp": kp, "plain": plain, "coded": coded,
                "coded_vs_plain": round(coded["ms"] / plain["ms"], 3),
                "layout_bytes_ratio": round(bytes_row["coded"] / bytes_row["plain"], 3),
                # a gain: the coded median lies below the plain one by more than three times the larger of the two spreads
                "gain": bool(plain["ms"] - coded["ms"] > 3.0 * max(plain["spread_ms"], coded["spread_ms"])),
            }
            print(name, k, json.dumps(out["spmm_t"][str(k)]), flush=True)
    return out


def step_solve(repeats):
    import numpy as np
    from krylovfspssa_amd import KfspContext, synth
    mdl = synth.toggle(1000, 1000)
    k, m, t, tol = 8, 30, 0.01, 1e-8
    # observables: indicator-like columns of different support (the backward solve propagates E[f(X_t) | X_0 = x])
    W = np.stack([synth.poisson_p0(mdl, 20.0 + 3.0 * j) for j in range(k)], axis=1)
    W /= W.max(axis=0)
    out = {"generator": "c2: toggle 1000 x 1000", "n": mdl.n, "k": k, "m": m, "t": t, "tol": tol, "adjoint": 1, "clamp": 0,
           "runs": {"0": [], "1": []}}
    with KfspContext(0) as ctx:
        ctx.set_option("dia_code", 1)
        ctx.set_matrix_box(mdl, store=True)
        ci = ctx.dia_code_info()
        out["code"] = {key: ci[key] for key in ("active", "width", "record_bytes", "dict_bytes", "diag_table_bytes")}
        assert ci["active"] == 1, ci
        ctx.set_option("block_dia_code", 1)
        res = {}
        for opt in (0, 1):                                # warm-up: allocations, code objects
            ctx.set_option(OPT, opt)
            ctx.set_block(W)
            ctx.expv_block(t / 10, tol, m, adjoint=True, clamp=False)
        for _ in range(repeats):
            for opt in (0, 1):
                ctx.set_option(OPT, opt)
                ctx.set_block(W)
                t0 = time.perf_counter()
                ws, st = ctx.expv_block(t, tol, m, adjoint=True, clamp=False)
                dt = time.perf_counter() - t0
                res[opt] = ctx.get_block()
                info = ctx.block_info()
                out["runs"][str(opt)].append({"wall_s": round(dt, 4), "nstep": st.nstep, "nreject": st.nreject, "block_products": st.nmult,
                                              "fmt": info["fmt"], "adjoint": info["adjoint"]})
        out["bit_identical"] = bool(np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64)))
    for opt in ("0", "1"):
        walls = [r["wall_s"] for r in out["runs"][opt]]
        out["wall_s_" + opt] = {"median": statistics.median(walls), "spread": round(max(walls) - min(walls), 4)}
    out["coded_vs_plain"] = round(out["wall_s_1"]["median"] / out["wall_s_0"]["median"], 3)
    return out


def run_step(step, args):
    return step_solve(3) if step == "solve" else step_products(step, [int(k) for k in args.ks.split(",")], args.reps, args.windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="c3,c3x,solve")
    ap.add_argument("--step", default=None, help="run this one step in-process and write its JSON to --out")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        line = json.dumps(run_step(args.step, args))
        with open(args.out or os.devnull, "w") as f:
            f.write(line + "\n")
        return 0
    out_path = args.out or os.path.join(HERE, "block_dia_code_adjoint.json")
    res = {"what": "transposed block product (adjoint = 1, block_dia_code = 1), block_dia_code_adjoint 0 / 1 alternating in one process "
                   "per generator; backward kfsp_expv_block on c2 at k = 8",
           "reps_per_window": args.reps, "windows": args.windows}
    rc = 0
    for step in args.steps.split(","):
        part = out_path + "." + step + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--ks", args.ks, "--reps", str(args.reps),
               "--windows", str(args.windows), "--out", part]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            res[step] = {"failed": rc}
            break                                         # nothing more on the device after a step that failed or hung
        with open(part) as f:
            res[step] = json.loads(f.read())
        os.remove(part)
    line = json.dumps(res)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
