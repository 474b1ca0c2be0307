"""What a resident target set costs (option block_target; DESIGN.md 12, "Target sets").  Writes profiles/block_target.json
and prints it as ONE JSON line.  On the toggle box of config 2 (synth.toggle(1000, 1000), 10^6 states, stored banded), a
30 % random set, k = 2 and 8 (kp = 2 and 8), m = 30:

  - whole solves: kfsp_expv_block(t = 0.1, tol = 1e-8, m = 30) with the set resident and with none, alternating, median of
    5: wall ms, steps, ms per step.  The two solves are different problems (Q = D A D against A: other step sizes), so the
    figure to compare is ms per step;
  - the no-set solve of ANOTHER TREE in the same session (--other-tree DIR: a checkout of the parent commit with its
    library built): both trees run the same child process (this file with --child, the package imported from the tree)
    in turns, 3 processes each; reported per tree: the median wall ms of each process and their spread;
  - per kernel (device times): run the kernel mode once per width, on its own, under a kernel trace,
        rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python profiles/block_target.py --kernels K
    (3 passes of kfsp_block_begin + kfsp_block_arnoldi(30) with the set and 3 without), then hand the stats files to
    --stats K=<..._kernel_stats.csv>: the TARGET instantiations of k_bcopy_nrm, k_bortho, k_bnorm against the plain ones.

    python profiles/block_target.py [--out FILE] [--t T] [--other-tree DIR] [--stats K=CSV ...]
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, TOL, M = 0.1, 1e-8, 30
KS = (2, 8)
KERNELS = ("k_bcopy_nrm", "k_bortho", "k_bnorm")


def package(tree):
    sys.path.insert(0, tree)
    import krylovfspssa_amd
    from krylovfspssa_amd import synth
    return krylovfspssa_amd.KfspContext, synth


def start_block(synth, mdl, k):
    W = np.zeros((mdl.n, k))
    for j in range(k):
        W[:, j] = synth.poisson_p0(mdl, 5.0 + 10.0 * j)
    return W


def flags_of(n):
    return (np.random.default_rng(17).random(n) < 0.3).astype(np.uint8)


def solve(ctx, W):
    ctx.set_block(W)
    t0 = time.perf_counter()
    ws, st = ctx.expv_block(T, TOL, M)
    wall = (time.perf_counter() - t0) * 1e3
    return {"wall_ms": wall, "nstep": st.nstep, "nreject": st.nreject, "ms_per_step": wall / (st.nstep + st.nreject)}


def median_of(recs):
    return {key: (round(float(np.median([r[key] for r in recs])), 4) if isinstance(recs[0][key], float) else recs[0][key])
            for key in recs[0]}


def child(tree):
    """no-set solves on the package of `tree`: one JSON line {k: [wall ms of 5 solves after a warm-up]}"""
    KfspContext, synth = package(tree)
    mdl = synth.toggle(1000, 1000)
    out = {}
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(mdl, store=True)
        for k in KS:
            W = start_block(synth, mdl, k)
            solve(ctx, W)
            out[str(k)] = [round(solve(ctx, W)["wall_ms"], 4) for _ in range(5)]
    print(json.dumps(out))


def kernels(k):
    """what a kernel trace should see: passes with the set and without at one width"""
    KfspContext, synth = package(ROOT)
    mdl = synth.toggle(1000, 1000)
    W = start_block(synth, mdl, k)
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(mdl, store=True)
        for flags in (flags_of(mdl.n), None):
            ctx.set_block_target(flags)
            ctx.set_block(W)
            for _ in range(3):
                ctx.block_begin(M)
                ctx.block_arnoldi(M)


def read_stats(path):
    """-> {kernel: {"plain_us": average, "target_us": average, "ratio": target / plain}} from a rocprofv3 kernel stats file"""
    avg = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for kern in KERNELS:
                for inst in ("true", "false"):
                    if f"{kern}<{inst}>" in row["Name"]:
                        avg[(kern, inst)] = (float(row["AverageNs"]) * 1e-3, int(row["Calls"]))
    out = {}
    for kern in KERNELS:
        (p, pc), (t, tc) = avg[(kern, "false")], avg[(kern, "true")]
        out[kern] = {"plain_us": round(p, 2), "target_us": round(t, 2), "calls_each": [pc, tc], "ratio": round(t / p, 4)}
    return out


def main():
    global T
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_target.json"))
    ap.add_argument("--other-tree", help="a checkout of another commit (its library built) for the no-set comparison")
    ap.add_argument("--stats", action="append", default=[], metavar="K=CSV", help="kernel stats of a --kernels K run")
    ap.add_argument("--t", type=float, default=T, help="end time of the solves (default 0.1: one step; larger: several)")
    ap.add_argument("--child", metavar="TREE", help="(internal) no-set solves on the package of TREE")
    ap.add_argument("--kernels", type=int, metavar="K", help="only the passes a kernel trace should see, k = K")
    args = ap.parse_args()
    T = args.t
    if args.child:
        return child(args.child)
    if args.kernels:
        return kernels(args.kernels)
    KfspContext, synth = package(ROOT)
    mdl = synth.toggle(1000, 1000)
    flags = flags_of(mdl.n)
    res = {"what": "target set (30 % random) against none on toggle(1000, 1000) stored banded, m = 30", "t": T, "tol": TOL, "m": M,
           "set_states": int(flags.sum()), "k": {}}
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(mdl, store=True)
        res["n"], res["format"] = ctx.n, ctx.layout_info()["format"]
        for k in KS:
            W = start_block(synth, mdl, k)
            runs = {"none": [], "set": []}
            for rep in range(6):                              # (the first round is the warm-up)
                for name in ("none", "set"):
                    ctx.set_block_target(flags if name == "set" else None)
                    rec = solve(ctx, W)
                    if rep:
                        runs[name].append(rec)
            none, with_set = median_of(runs["none"]), median_of(runs["set"])
            res["k"][str(k)] = {"solve": {"none": none, "set": with_set,
                                          "ms_per_step_ratio_set_over_none": round(with_set["ms_per_step"] / none["ms_per_step"], 4)}}
    if args.other_tree:
        procs = {"this": [], "other": []}
        for _ in range(3):
            for name, tree in (("other", os.path.abspath(args.other_tree)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True, text=True, check=True)
                procs[name].append(json.loads(r.stdout.strip().split("\n")[-1]))
        for k in KS:
            rec = {}
            for name in procs:
                meds = [float(np.median(p[str(k)])) for p in procs[name]]
                rec[name] = {"median_ms_of_each_process": [round(x, 4) for x in meds], "median_ms": round(float(np.median(meds)), 4),
                             "spread_ms": round(max(meds) - min(meds), 4)}
            rec["this_over_other"] = round(rec["this"]["median_ms"] / rec["other"]["median_ms"], 4)
            res["k"][str(k)]["no_set_solve_against_other_tree"] = rec
    for item in args.stats:
        k, path = item.split("=", 1)
        res["k"][str(int(k))]["kernels"] = read_stats(path)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
