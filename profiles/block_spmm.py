"""Block product and block solve timing (several start vectors at once).  Prints ONE JSON line:

  - c3 stored (repressilator box 171^3, box_store = 1) and the 10^7-state Goutsias FSP of bench.py --fsp (internal state
    order): kfsp_spmv_bench at k = 1 against kfsp_spmm_bench at k = 1, 2, 4, 8, 16 (warmed up), ms per block and per
    vector, layout bytes per block (kfsp_matrix_bytes - 16 B per row + 16 kp B per row) and the fraction of 8 TB/s on them;
  - kfsp_expv_block wall time per column at k = 1 and k = 8 on the c2 toggle box (1000 x 1000, stored), with step counts.

    python profiles/block_spmm.py [--reps 50] [--no-fsp]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from krylovfspssa_amd import KfspContext, synth  # noqa: E402

PEAK = 8.0e12
KS = (1, 2, 4, 8, 16)


def kp_of(k):
    return 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16


def products(ctx, reps, rng):
    n = ctx.n
    rows = ctx.matrix_info()["rows"]
    gen_bytes = ctx.matrix_bytes() - 16 * rows            # the generator stream + DIAG (x and y are per column)
    ctx.spmv_bench(5)
    ms1 = ctx.spmv_bench(reps) / reps
    out = {"n": n, "format": ctx.layout_info()["format"], "matrix_bytes": ctx.matrix_bytes(),
           "spmv_ms": round(ms1, 5), "spmv_frac_of_peak": round(ctx.matrix_bytes() / (ms1 * 1e-3) / PEAK, 3), "spmm": {}}
    for k in KS:
        ctx.set_block(rng.random((n, k)))
        ctx.spmm_bench(5)
        ms = ctx.spmm_bench(reps) / reps
        b = gen_bytes + 16 * kp_of(k) * rows
        out["spmm"][str(k)] = {"kp": kp_of(k), "ms_per_block": round(ms, 5), "ms_per_vector": round(ms / k, 5),
                               "per_vector_vs_spmv": round(ms / k / ms1, 3), "layout_bytes": int(b),
                               "frac_of_peak": round(b / (ms * 1e-3) / PEAK, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-fsp", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res = {"what": "block products (kfsp_spmm_bench) vs single products (kfsp_spmv_bench), and kfsp_expv_block per column"}
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(synth.repressilator(dims=(171, 171, 171)), store=True)
        res["c3_stored"] = products(ctx, args.reps, rng)
    if not args.no_fsp:
        fsp = synth.GoutsiasEllipsoid()
        with KfspContext(0) as ctx:
            ctx.set_option("state_order_min", 1)
            ctx.set_option("state_order_products", 0)
            ctx.set_option("m_max", 8)
            ctx.set_state_coords(fsp.state)
            ctx.set_matrix_ell(*fsp.ell())
            res["fsp_goutsias_1e7"] = products(ctx, args.reps, rng)
    mdl = synth.toggle(1000, 1000)
    W = np.zeros((mdl.n, 8))
    for j in range(8):
        W[:, j] = synth.poisson_p0(synth.toggle(1000, 1000), 5.0 + 10.0 * j)
    solve = {}
    with KfspContext(0) as ctx:
        ctx.set_matrix_box(mdl, store=True)
        for k in (1, 8):
            ctx.set_block(W[:, :k])
            ctx.expv_block(0.01, 1e-8, 30)                 # warm-up (allocations, code objects)
            ctx.set_block(W[:, :k])
            t0 = time.perf_counter()
            ws, st = ctx.expv_block(0.1, 1e-8, 30)
            dt = time.perf_counter() - t0
            solve[str(k)] = {"wall_s": round(dt, 4), "wall_s_per_column": round(dt / k, 4), "nstep": st.nstep, "nreject": st.nreject,
                             "block_products": st.nmult, "min_mass": float(ws.min())}
    res["expv_block_c2_toggle_stored"] = {"t": 0.1, "tol": 1e-8, "m": 30, "runs": solve}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
