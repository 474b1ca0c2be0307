"""Block product on MATRIX-FREE boxes (option block_box, k_spmm_box; DESIGN.md 12, "Matrix-free boxes").  Writes ONE JSON object
(--out, default profiles/block_box.json) and prints it.  Per box - c3 (repressilator 171^3), c3x (216^3), c5s (22^5 x 3) - and
k = 1, 2, 4, 8, 16, all on the same box and the same X in one run, HIP-event windows of --reps launches, median of --windows:

  (a) kfsp_spmm_bench matrix-free: ms per block and per vector;
  (b) one matrix-free kfsp_spmv_bench product;
  (c) kfsp_spmm_bench on the same box stored (box_store = 1) at the same k, and the stored single product;
  (d) c3 only: kfsp_expv_block at k = 8, m = 30, matrix-free against stored (wall time, step counts).

    python profiles/block_box.py [--boxes c3,c3x,c5s] [--ks 1,2,4,8,16] [--reps 200] [--windows 5] [--no-stored] [--no-solve]

The counter passes (one counter per run, no tracing) use the short form:
    rocprofv3 --pmc FETCH_SIZE -d <dir> -o <name> --output-format csv -- \\
        python profiles/block_box.py --boxes c3 --ks 2,8 --reps 3 --windows 1 --no-stored --no-solve --out /dev/null
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from krylovfspssa_amd import KfspContext, synth  # noqa: E402

BOXES = {
    "c3": lambda: synth.repressilator(dims=(171, 171, 171)),
    "c3x": lambda: synth.repressilator(dims=(216, 216, 216)),
    "c5s": lambda: synth.birth_death((22, 22, 22, 22, 22, 3)),
}


def kp_of(k):
    return 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16


def median_ms(bench, reps, windows):
    bench(5)
    return statistics.median(bench(reps) / reps for _ in range(windows))


def products(ctx, X, ks, reps, windows):
    out = {"format": ctx.layout_info()["format"], "spmv_ms": round(median_ms(ctx.spmv_bench, reps, windows), 5), "spmm": {}}
    for k in ks:
        ctx.set_block(X[:, :k])
        ms = median_ms(ctx.spmm_bench, reps, windows)
        out["spmm"][str(k)] = {"kp": kp_of(k), "ms_per_block": round(ms, 5), "ms_per_vector": round(ms / k, 5),
                               "per_vector_vs_spmv": round(ms / k / out["spmv_ms"], 3)}
    return out


def solve(ctx, W, t, tol, m):
    ctx.set_block(W)
    ctx.expv_block(t / 10, tol, m)                         # warm-up (allocations, code objects)
    ctx.set_block(W)
    t0 = time.perf_counter()
    ws, st = ctx.expv_block(t, tol, m)
    dt = time.perf_counter() - t0
    return {"wall_s": round(dt, 4), "nstep": st.nstep, "nreject": st.nreject, "block_products": st.nmult, "min_mass": float(ws.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="c3,c3x,c5s")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-stored", action="store_true")
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "block_box.json"))
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    res = {"what": "block products on matrix-free boxes (block_box = 1) vs one matrix-free product and vs the stored block",
           "reps_per_window": args.reps, "windows": args.windows}
    for name in args.boxes.split(","):
        mdl = BOXES[name]()
        X = np.random.default_rng(0).random((mdl.n, max(ks)))
        box = {"n": mdl.n, "dims": list(mdl.dims)}
        with KfspContext(0) as ctx:
            ctx.set_option("block_box", 1)
            ctx.set_matrix_box(mdl, store=False)
            box["matrix_free"] = products(ctx, X, ks, args.reps, args.windows)
        if not args.no_stored:
            with KfspContext(0) as ctx:
                ctx.set_matrix_box(mdl, store=True)
                box["stored"] = products(ctx, X, ks, args.reps, args.windows)
            for k in ks:
                a, c = box["matrix_free"]["spmm"][str(k)], box["stored"]["spmm"][str(k)]
                a["vs_stored_block"] = round(a["ms_per_block"] / c["ms_per_block"], 3)
        res[name] = box
        print(name, json.dumps(box), flush=True)
    if not args.no_solve and "c3" in args.boxes.split(","):
        mdl = BOXES["c3"]()
        W = np.stack([synth.poisson_p0(mdl, 5.0 + 4.0 * j) for j in range(8)], axis=1)
        runs = {}
        for form, store in (("matrix_free", False), ("stored", True)):
            with KfspContext(0) as ctx:
                ctx.set_option("block_box", 1)
                ctx.set_matrix_box(mdl, store=store)
                runs[form] = solve(ctx, W, 0.02, 1e-8, 30)
        res["expv_block_c3_k8"] = {"t": 0.02, "tol": 1e-8, "m": 30, "runs": runs}
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
