"""What the host-side refactor of the block path (block_plan, kfsp_block_plan.h; DESIGN.md 12, "One rule, one record, two
files") is measured with, on the parent commit and on this tree alike (profiles/block_plan_ab.sh runs both):

  python profiles/block_plan.py launches [--root TREE]   the target of one rocprofv3 --kernel-trace --stats run: one A X and one
                                                          A^T X at k = 4 on steps a, c, e, f and g of
                                                          tests/test_gpu_block_sequence.py, one kfsp_expv_block on step a
  python profiles/block_plan.py spmm [--root TREE]       one JSON line: ms per block product of kfsp_spmm_bench(200) at k = 4 on
                                                          the benchmark's generator (repressilator 171^3, stored), 5 windows

TREE: the checkout whose krylovfspssa_amd (and built library) is loaded; default this one."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def launches():
    import numpy as np
    from krylovfspssa_amd import KfspContext
    from tests import test_gpu_block_sequence as S
    steps = {s[0][0]: s for s in S._steps()}
    rng = np.random.default_rng(3)
    for key in "acefg":
        n = steps[key][2]
        with KfspContext(0) as c:
            S._apply(c, steps[key])
            X = rng.standard_normal((n, 4))
            c.spmm(X)
            fwd = c.block_info()
            c.set_option("block_dia_code_adjoint", 1)
            c.spmm(X, adjoint=True)
            print(steps[key][0], fwd, c.block_info(), flush=True)
            if key == "a":
                W = rng.random((n, 4))
                c.set_block(W / W.sum(axis=0))
                _, st = c.expv_block(1e-3, 1e-8, m=10)
                print("expv_block", st.nstep, st.nmult, c.block_info(), flush=True)


def spmm():
    import numpy as np
    from krylovfspssa_amd import KfspContext, synth
    mdl = synth.repressilator(dims=(171, 171, 171))
    with KfspContext(0) as c:
        c.set_matrix_box(mdl, store=True)
        c.set_block(np.random.default_rng(0).random((mdl.n, 4)))
        c.spmm_bench(20)
        ms = [c.spmm_bench(200) / 200 for _ in range(5)]
        print(json.dumps({"n": mdl.n, "k": 4, "ms_per_product": sorted(ms)[2], "windows_ms": ms, "info": c.block_info()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launches", "spmm"])
    ap.add_argument("--root", default=os.path.dirname(HERE))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))          # tests/
    sys.path.insert(0, os.path.abspath(args.root))     # krylovfspssa_amd of the tree under measurement
    launches() if args.what == "launches" else spmm()
