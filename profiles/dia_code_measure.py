"""build time of the coded image and product time plain / coded, c2 and c3 (and nt on / off for the coded kernel)

    python3 profiles/dia_code_measure.py <result.json>     (kept as profiles/dia_code_measure.json)"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from krylovfspssa_amd import KfspContext, synth

out = {}
for name, mdl in (("c2", synth.toggle(1000, 1000)), ("c3", synth.repressilator(171))):
    rowptr, col, val = mdl.csr_rows()
    x = np.random.default_rng(12345).random(mdl.n)
    r = {}
    ys = {}
    for label, dc, nt in (("plain", 0, -1), ("coded", 1, -1), ("coded_nt0", 1, 0), ("coded_nt1", 1, 1), ("plain_again", 0, -1)):
        with KfspContext(0) as c:
            c.set_option("m_max", 8)
            c.set_option("dia_code", dc)
            c.set_option("nt_loads", nt)
            c.set_matrix_csr(mdl.n, rowptr, col, val)
            ci = c.dia_code_info()
            builds = [ci["build_us"]]
            if dc and label == "coded":
                for _ in range(3):                      # warm builds: buffers exist
                    c.set_matrix_csr(mdl.n, rowptr, col, val)
                    builds.append(c.dia_code_info()["build_us"])
            c.set_vector(x)
            c.begin_step()
            c.spmv_bench(20)
            ms = sorted(c.spmv_bench(200) / 200 for _ in range(5))
            ys[label] = c.spmv_w()
            r[label] = {"us_min": round(ms[0] * 1e3, 3), "us_med": round(ms[2] * 1e3, 3), "us_max": round(ms[4] * 1e3, 3),
                        "bytes": c.matrix_bytes(), "info": ci, "build_us": builds, "layout": c.layout_info()}
            print(name, label, r[label], flush=True)
    r["bit_identical"] = bool(np.array_equal(ys["plain"].view(np.uint64), ys["coded"].view(np.uint64)))
    print(name, "bit identical", r["bit_identical"], flush=True)
    out[name] = r
json.dump(out, open(sys.argv[1], "w"), indent=1)
