"""Block product on dictionary-coded banded generators (option block_dia_code, k_spmm_diac; DESIGN.md 12, "Coded banded
generators").  Writes ONE JSON object (--out, default profiles/block_dia_code.json) and prints it.

Steps, each in a child process of its own under its own time limit (the parent never opens the device; a step that fails or
runs out of time ends the run there):

  c3, c3x   the repressilator box 171^3 (5.0e6 states) and 216^3 (1.0e7), stored as diagonals on the device, dia_code auto
            (both lie beyond the Infinity Cache: the coded image builds itself).  For k = 1, 2, 4, 8, 16, in ONE process
            and on one resident block: kfsp_spmm_bench with block_dia_code alternating 0, 1, 0, 1, ... - HIP-event windows
            of --reps launches, --windows windows per setting, median and spread (max - min) of each - and
            kfsp_spmv_bench, the coded single product, timed the same way in the same process.  The plain block of the
            same process is the baseline of every ratio.
  solve     kfsp_expv_block on c2 (toggle 1000 x 1000, dia_code = 1: below the Infinity Cache the image is built on
            request only) at k = 8, m = 30, the two settings alternating; wall time, steps, and whether W came out
            bit-identical.

    python profiles/block_dia_code.py [--steps c3,c3x,solve] [--ks 1,2,4,8,16] [--reps 200] [--windows 5] [--limit 420]

The counter passes take one step in-process (--step), few launches, one counter per run and no tracing beside it:

    rocprofv3 --pmc FETCH_SIZE -d <dir> -o fetch --output-format csv -- \\
        python profiles/block_dia_code.py --step c3 --ks 2,4,8,16 --reps 3 --windows 1 --out /dev/null
    rocprofv3 --pmc WRITE_SIZE -d <dir> -o write --output-format csv -- (the same)
    python profiles/block_dia_code.py --pmc <dir>/*/*counter_collection.csv      -> profiles/block_dia_code_pmc_fetch.csv
"""
import argparse
import csv
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


def kp_of(k):
    return 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16


def windows_ms(bench, reps, windows):
    return [bench(reps) / reps for _ in range(windows)]


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
        out.update(format=lay["format"], rows=rows, diagonals=nd, code={key: ci[key] for key in ("active", "width", "record_bytes", "dict_bytes")})
        assert ci["active"] == 1, ci
        ctx.set_vector(X[:, 0])
        ctx.begin_step()
        ctx.spmv_bench(5)
        out["spmv_coded"] = summary(windows_ms(ctx.spmv_bench, reps, windows))
        out["spmm"] = {}
        for k in ks:
            kp = kp_of(k)
            ctx.set_block(X[:, :k])
            ms = {0: [], 1: []}
            for opt in (0, 1):
                ctx.set_option("block_dia_code", opt)
                ctx.spmm_bench(5)
            for _ in range(windows):
                for opt in (0, 1):
                    ctx.set_option("block_dia_code", opt)
                    ms[opt].append(ctx.spmm_bench(reps) / reps)
                    # (only a product under the option writes the slot: 9 says the coded kernel ran)
                    assert opt == 0 or ctx.block_info()["fmt"] == 9, ctx.block_info()
            plain, coded = summary(ms[0]), summary(ms[1])
            bytes_row = {"plain": 8 * nd + 8 + 16 * kp, "coded": rec + 8 + 16 * kp}
            for s, key in ((plain, "plain"), (coded, "coded")):
                s["ms_per_vector"] = round(s["ms"] / k, 5)
                s["layout_bytes_per_row"] = bytes_row[key]
                s["fraction_of_8TBps"] = round(bytes_row[key] * rows / (s["ms"] * 1e-3) / HBM_BYTES_PER_S, 3)
            out["spmm"][str(k)] = {
                "kp": kp, "plain": plain, "coded": coded,
                "coded_vs_plain": round(coded["ms"] / plain["ms"], 3),
                "coded_vs_k_coded_spmv": round(coded["ms"] / (k * out["spmv_coded"]["ms"]), 3),
                "plain_vs_k_coded_spmv": round(plain["ms"] / (k * out["spmv_coded"]["ms"]), 3),
                # a gain: the coded median lies below the plain one by more than the larger of the two spreads
                "gain": bool(plain["ms"] - coded["ms"] > max(plain["spread_ms"], coded["spread_ms"])),
            }
            print(name, k, json.dumps(out["spmm"][str(k)]), flush=True)
    return out


def step_solve(repeats):
    import numpy as np
    from krylovfspssa_amd import KfspContext, synth
    mdl = synth.toggle(1000, 1000)
    k, m, t, tol = 8, 30, 0.01, 1e-8
    W = np.stack([synth.poisson_p0(mdl, 20.0 + 3.0 * j) for j in range(k)], axis=1)
    out = {"generator": "c2: toggle 1000 x 1000", "n": mdl.n, "k": k, "m": m, "t": t, "tol": tol, "runs": {"0": [], "1": []}}
    with KfspContext(0) as ctx:
        ctx.set_option("dia_code", 1)
        ctx.set_matrix_box(mdl, store=True)
        ci = ctx.dia_code_info()
        out["code"] = {key: ci[key] for key in ("active", "width", "record_bytes", "dict_bytes")}
        assert ci["active"] == 1, ci
        res = {}
        for opt in (0, 1):                                # warm-up: allocations, code objects
            ctx.set_option("block_dia_code", opt)
            ctx.set_block(W)
            ctx.expv_block(t / 10, tol, m)
        for _ in range(repeats):
            for opt in (0, 1):
                ctx.set_option("block_dia_code", opt)
                ctx.set_block(W)
                t0 = time.perf_counter()
                ws, st = ctx.expv_block(t, tol, m)
                dt = time.perf_counter() - t0
                res[opt] = ctx.get_block()
                out["runs"][str(opt)].append({"wall_s": round(dt, 4), "nstep": st.nstep, "nreject": st.nreject, "block_products": st.nmult,
                                              "fmt": ctx.block_info()["fmt"], "min_mass": float(ws.min())})
        out["bit_identical"] = bool(np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64)))
    for opt in ("0", "1"):
        walls = [r["wall_s"] for r in out["runs"][opt]]
        out["wall_s_" + opt] = {"median": statistics.median(walls), "spread": round(max(walls) - min(walls), 4)}
    out["coded_vs_plain"] = round(out["wall_s_1"]["median"] / out["wall_s_0"]["median"], 3)
    return out


def run_step(step, args):
    return step_solve(3) if step == "solve" else step_products(step, [int(k) for k in args.ks.split(",")], args.reps, args.windows)


def pmc_summary(paths, out_path):
    """rocprofv3 counter CSVs (KB per dispatch) -> one row per kernel and counter; FETCH_SIZE doubled: on gfx950 it counts a
    wide coalesced read at half its bytes, WRITE_SIZE is exact"""
    acc = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if "k_spmm" not in name:
                    continue
                acc.setdefault((name, row["Counter_Name"]), []).append(float(row["Counter_Value"]))
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "setting", "kp", "counter", "dispatches", "median_counter_KB", "bytes_per_dispatch", "doubled"])
        for (name, counter), vals in sorted(acc.items()):
            coded = "k_spmm_diac" in name
            kp = int(name.split("<")[1].split(",")[0])
            med = statistics.median(vals)
            factor = 2 if counter == "FETCH_SIZE" else 1
            w.writerow([name.replace("kfsp::(anonymous namespace)::", ""), "block_dia_code=1" if coded else "block_dia_code=0", kp, counter,
                        len(vals), round(med, 3), int(med * 1024 * factor), "yes" if factor == 2 else "no"])
    print(open(out_path).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="c3,c3x,solve")
    ap.add_argument("--step", default=None, help="run this one step in-process and write its JSON to --out")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--pmc", nargs="+", default=None, help="summarise these rocprofv3 counter CSVs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pmc:
        pmc_summary(args.pmc, args.out or os.path.join(HERE, "block_dia_code_pmc_fetch.csv"))
        return 0
    if args.step:
        line = json.dumps(run_step(args.step, args))
        with open(args.out or os.devnull, "w") as f:
            f.write(line + "\n")
        return 0
    out_path = args.out or os.path.join(HERE, "block_dia_code.json")
    res = {"what": "forward block product, block_dia_code 0 / 1 alternating in one process per generator; kfsp_spmv_bench beside it; "
                   "kfsp_expv_block on c2 at k = 8",
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
