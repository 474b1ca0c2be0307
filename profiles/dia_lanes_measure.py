"""The lane path of the folded banded product (option dia_code_lanes) on c3 and c3x: product time with the
+-1 pairs of x loaded (dia_code_lanes = 0) and taken from the neighbour lanes (1) - ONE context per workload, the option is
read at every launch, so the two sides alternate window by window on the same generator in the same process: 200-launch
HIP-event windows, 5 per side, median / min / max - and whether the two products are the same bits.  `stream`: the same
with DIAG as a stream (dia_code_diag = 0), the parent's default kernel, in a context of its own.

    python3 profiles/dia_lanes_measure.py <result.json> [c3 c3x]     (kept as profiles/dia_lanes_measure.json)"""
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
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        c.set_vector(x)
        c.begin_step()
        c.spmv_bench(20)
        win = {0: [], 1: []}
        for _ in range(5):
            for lanes in (0, 1):
                c.set_option("dia_code_lanes", lanes)
                win[lanes].append(c.spmv_bench(200) / 200 * 1e3)
        for lanes, label in ((0, "loads"), (1, "lanes")):
            c.set_option("dia_code_lanes", lanes)
            ys[label] = c.spmv_w()
            w = sorted(win[lanes])
            r[label] = {"us_windows": [round(v, 3) for v in win[lanes]], "us_min": round(w[0], 3), "us_med": round(w[2], 3),
                        "us_max": round(w[4], 3), "info": c.dia_code_info(), "bytes": c.matrix_bytes()}
            print(wl, label, r[label], flush=True)
    with KfspContext(0) as c:
        c.set_option("m_max", 8)
        c.set_option("dia_code_diag", 0)
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        c.set_vector(x)
        c.begin_step()
        c.spmv_bench(20)
        w = [c.spmv_bench(200) / 200 * 1e3 for _ in range(5)]
        ys["stream"] = c.spmv_w()
        r["stream"] = {"us_windows": [round(v, 3) for v in w], "us_min": round(min(w), 3), "us_med": round(sorted(w)[2], 3),
                       "us_max": round(max(w), 3), "info": c.dia_code_info(), "bytes": c.matrix_bytes()}
        print(wl, "stream", r["stream"], flush=True)
    spread = max(r["loads"]["us_max"] - r["loads"]["us_min"], r["lanes"]["us_max"] - r["lanes"]["us_min"])
    r["gain_us"] = round(r["loads"]["us_med"] - r["lanes"]["us_med"], 3)
    r["larger_spread_us"] = round(spread, 3)
    r["lanes_clear_the_spread"] = bool(r["gain_us"] > spread)
    r["bit_identical"] = bool(np.array_equal(ys["loads"].view(np.uint64), ys["lanes"].view(np.uint64)) and
                              np.array_equal(ys["stream"].view(np.uint64), ys["lanes"].view(np.uint64)))
    print(wl, "gain", r["gain_us"], "us, larger spread", r["larger_spread_us"], "us, clears it:", r["lanes_clear_the_spread"],
          "bit identical", r["bit_identical"], flush=True)
    out[wl] = r
json.dump(out, open(sys.argv[1], "w"), indent=1)
