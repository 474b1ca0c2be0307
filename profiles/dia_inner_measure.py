"""The interior path of the folded banded product (option dia_code_inner) on c3 and c3x: product time with
every trip through rows_dia (dia_code_inner = 0, `present`) and with the interior trips through rows_dia_inner (1, `inner`) -
ONE context per workload, the option is read at every launch, so the two sides alternate window by window on the same
generator in the same process: 200-launch HIP-event windows, 5 per side, median / min / max - and whether the two products
are the same bits.

    python3 profiles/dia_inner_measure.py <result.json> [c3 c3x]     (kept as profiles/dia_inner_measure.json)"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from krylovfspssa_amd import KfspContext, synth

SIDE = {"c3": 171, "c3x": 216}
out = {}
for wl in (sys.argv[2:] or ["c3", "c3x"]):
    mdl = synth.repressilator(SIDE[wl])
    rowptr, col, val = mdl.csr_rows()
    x = np.random.default_rng(12345).random(mdl.n)
    r, ys = {}, {}
    with KfspContext(0) as c:
        c.set_option("m_max", 8)
        c.set_option("dia_code_diag", -1)
        c.set_option("dia_code_lanes", 0)
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        c.set_vector(x)
        c.begin_step()
        c.spmv_bench(20)
        win = {0: [], 1: []}
        for _ in range(5):
            for inner in (0, 1):
                c.set_option("dia_code_inner", inner)
                win[inner].append(c.spmv_bench(200) / 200 * 1e3)
        for inner, label in ((0, "present"), (1, "inner")):
            c.set_option("dia_code_inner", inner)
            ys[label] = c.spmv_w()
            w = sorted(win[inner])
            r[label] = {"us_windows": [round(v, 3) for v in win[inner]], "us_min": round(w[0], 3), "us_med": round(w[2], 3),
                        "us_max": round(w[4], 3), "info": c.dia_code_info(), "bytes": c.matrix_bytes()}
            print(wl, label, r[label], flush=True)
    spread = max(r["present"]["us_max"] - r["present"]["us_min"], r["inner"]["us_max"] - r["inner"]["us_min"])
    r["gain_us"] = round(r["present"]["us_med"] - r["inner"]["us_med"], 3)
    r["larger_spread_us"] = round(spread, 3)
    r["inner_clears_the_spread"] = bool(r["gain_us"] > spread)
    r["bit_identical"] = bool(np.array_equal(ys["present"].view(np.uint64), ys["inner"].view(np.uint64)))
    print(wl, "gain", r["gain_us"], "us, larger spread", r["larger_spread_us"], "us, clears it:", r["inner_clears_the_spread"],
          "bit identical", r["bit_identical"], flush=True)
    out[wl] = r
json.dump(out, open(sys.argv[1], "w"), indent=1)
