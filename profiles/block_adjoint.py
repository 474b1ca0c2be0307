"""The transposed block product against the forward one (option adjoint; DESIGN.md 12, "Backward solves").  Writes ONE JSON
object (--out, default profiles/block_adjoint.json) and prints it.  Per generator - c3 stored (repressilator 171^3,
box_store = 1: k_spmm_t), c3 matrix-free under block_box (k_spmm_box_t) and an SSA-ordered Goutsias FSP of about 10^6 states
under the internal state order (k_spmm_ell_t) - and k = 1, 2, 4, 8, 16: kfsp_spmm_bench with adjoint = 0 and 1 ALTERNATING in one
process on one context and one resident block, HIP-event windows of --reps launches, median of --windows, after a warm-up
of both; ms per block for either direction and their ratio.

    python profiles/block_adjoint.py [--gens c3_stored,c3_box,fsp] [--ks 1,2,4,8,16] [--reps 200] [--windows 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from krylovfspssa_amd import KfspContext, synth  # noqa: E402


def c3():
    return synth.repressilator(dims=(171, 171, 171))


def set_c3_stored(ctx):
    ctx.set_matrix_box(c3(), store=True)


def set_c3_box(ctx):
    ctx.set_option("block_box", 1)
    ctx.set_matrix_box(c3(), store=False)


def set_fsp(ctx):
    fsp = synth.GoutsiasEllipsoid(center=(28, 23, 9), axes=(51, 42, 37))
    ctx.set_option("state_order_min", 1)
    ctx.set_option("state_order_products", 0)
    ctx.set_option("m_max", 8)
    ctx.set_state_coords(fsp.state)
    ctx.set_matrix_ell(*fsp.ell())


GENS = {"c3_stored": set_c3_stored, "c3_box": set_c3_box, "fsp": set_fsp}


def alternate(ctx, reps, windows):
    """-> (forward ms, adjoint ms) per block: the two directions take turns window by window"""
    ms = {0: [], 1: []}
    for adj in (0, 1):
        ctx.set_option("adjoint", adj)
        ctx.spmm_bench(5)
    for _ in range(windows):
        for adj in (0, 1):
            ctx.set_option("adjoint", adj)
            ms[adj].append(ctx.spmm_bench(reps) / reps)
    ctx.set_option("adjoint", 0)
    return statistics.median(ms[0]), statistics.median(ms[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gens", default="c3_stored,c3_box,fsp")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "block_adjoint.json"))
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    res = {"what": "kfsp_spmm_bench, adjoint = 0 / 1 alternating on one context, ms per block product",
           "reps_per_window": args.reps, "windows": args.windows}
    for name in args.gens.split(","):
        with KfspContext(0) as ctx:
            GENS[name](ctx)
            X = np.random.default_rng(0).random((ctx.n, max(ks)))
            gen = {"n": ctx.n, "format": ctx.layout_info()["format"], "state_order": ctx.state_order_active(), "k": {}}
            for k in ks:
                ctx.set_block(X[:, :k])
                fwd, adj = alternate(ctx, args.reps, args.windows)
                gen["k"][str(k)] = {"forward_ms": round(fwd, 5), "adjoint_ms": round(adj, 5), "adjoint_vs_forward": round(adj / fwd, 3)}
        res[name] = gen
        print(name, json.dumps(gen), flush=True)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
