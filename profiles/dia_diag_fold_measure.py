"""DIAG folded into the coded records' spare bits (option dia_code_diag) on c3: build time of the coded image
with and without the fold (cold, then three warm builds), product time of both (200-launch HIP-event windows, median of 5,
alternating so that neither side owns the warm card) and whether the two products are the same bits

    python3 profiles/dia_diag_fold_measure.py <result.json>     (kept as profiles/dia_diag_fold_measure.json)"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from krylovfspssa_amd import KfspContext, synth

mdl = synth.repressilator(171)
rowptr, col, val = mdl.csr_rows()
x = np.random.default_rng(12345).random(mdl.n)
r, ys = {}, {}
for label, fold in (("stream", 0), ("folded", -1), ("stream_again", 0), ("folded_again", -1)):
    with KfspContext(0) as c:
        c.set_option("m_max", 8)
        c.set_option("dia_code_diag", fold)
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        builds = [c.dia_code_info()["build_us"]]
        for _ in range(3):                              # warm builds: buffers exist
            c.set_matrix_csr(mdl.n, rowptr, col, val)
            builds.append(c.dia_code_info()["build_us"])
        ci = c.dia_code_info()
        c.set_vector(x)
        c.begin_step()
        c.spmv_bench(20)
        ms = sorted(c.spmv_bench(200) / 200 for _ in range(5))
        ys[label] = c.spmv_w()
        r[label] = {"us_min": round(ms[0] * 1e3, 3), "us_med": round(ms[2] * 1e3, 3), "us_max": round(ms[4] * 1e3, 3),
                    "bytes": c.matrix_bytes(), "info": ci, "build_us": builds, "layout": c.layout_info()}
        print(label, r[label], flush=True)
r["bit_identical"] = bool(np.array_equal(ys["stream"].view(np.uint64), ys["folded"].view(np.uint64)))
print("bit identical", r["bit_identical"], flush=True)
json.dump({"c3": r}, open(sys.argv[1], "w"), indent=1)
