"""Block product on a MULTI-FACTOR matrix-free box (option block_box = 2, k_spmm_boxg; DESIGN.md 12, "Multi-factor boxes").
Writes ONE JSON object (--out, default profiles/block_box_generic.json) and prints it.  Workload: a Goutsias box of about
10^7 states (two bimolecular reactions, one reaction moving three species, jumps of 2: no single-factor form).  For
k = 1, 2, 4, 8, 16, all on the same box and the same X in one process, HIP-event windows of --reps launches, median of
--windows:

  (a) kfsp_spmm_bench, the generic block product under block_box = 2: ms per block and per vector;
  (b) k times the single-vector format-3 product (kfsp_spmv_bench) on the same context;
  (c) kfsp_spmm_bench of the same box stored as diagonals (box_store = 1) at the same k.

    python profiles/block_box_generic.py [--dims 30,30,32,7,7,7] [--ks 1,2,4,8,16] [--reps 50] [--windows 5] [--adjoint] [--no-stored]

--adjoint adds the transposed product (k_spmm_boxg_t against k_spmm_t on the stored box)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from krylovfspssa_amd import KfspContext, synth  # noqa: E402


def kp_of(k):
    return 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16


def median_ms(bench, reps, windows):
    bench(3)
    return statistics.median(bench(reps) / reps for _ in range(windows))


def blocks(ctx, X, ks, reps, windows, adjoint):
    out = {}
    for k in ks:
        ctx.set_block(X[:, :k])
        row = {"kp": kp_of(k)}
        for name, on in (("forward", 0), ("adjoint", 1)):
            if on and not adjoint:
                continue
            ctx.set_option("adjoint", on)
            try:
                ms = median_ms(ctx.spmm_bench, reps, windows)
            finally:
                ctx.set_option("adjoint", 0)
            row[name] = {"ms_per_block": round(ms, 5), "ms_per_vector": round(ms / k, 5)}
        out[str(k)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="30,30,32,7,7,7")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--adjoint", action="store_true")
    ap.add_argument("--no-stored", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "block_box_generic.json"))
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    mdl = synth.goutsias_box(tuple(int(d) for d in args.dims.split(",")))
    X = np.random.default_rng(0).random((mdl.n, max(ks)))
    res = {"what": "generic matrix-free block product (block_box = 2) vs k format-3 products and vs the stored block",
           "box": "goutsias", "dims": list(mdl.dims), "n": mdl.n, "reps_per_window": args.reps, "windows": args.windows}
    with KfspContext(0) as ctx:
        ctx.set_option("block_box", 2)
        ctx.set_matrix_box(mdl, store=False)
        res["format"] = ctx.layout_info()["format"]
        res["spmv_ms"] = round(median_ms(ctx.spmv_bench, args.reps, args.windows), 5)
        res["matrix_free"] = blocks(ctx, X, ks, args.reps, args.windows, args.adjoint)
    print(json.dumps(res), flush=True)
    if not args.no_stored:
        with KfspContext(0) as ctx:
            ctx.set_matrix_box(mdl, store=True)
            res["stored_format"] = ctx.layout_info()["format"]
            res["stored_spmv_ms"] = round(median_ms(ctx.spmv_bench, args.reps, args.windows), 5)
            res["stored"] = blocks(ctx, X, ks, args.reps, args.windows, args.adjoint)
    for k in ks:
        a = res["matrix_free"][str(k)]
        for d in ("forward", "adjoint"):
            if d not in a:
                continue
            a[d]["vs_k_spmv"] = round(a[d]["ms_per_block"] / (k * res["spmv_ms"]), 3)
            if "stored" in res:
                a[d]["vs_stored_block"] = round(a[d]["ms_per_block"] / res["stored"][str(k)][d]["ms_per_block"], 3)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
