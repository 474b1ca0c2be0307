"""Reduce the FETCH_SIZE / WRITE_SIZE passes of profiles/pmc_target.py (run with --no-time: every case is exactly 5
launches of the product kernel) for the dictionary-coded banded form: per case the median HBM bytes per launch -
FETCH_SIZE (KiB) x 1024 x 2 (the counter reports half the bytes on this part, guides: MI355X_MICROARCH.md; the
calibration passes of the earlier rounds measured the same 2.0), WRITE_SIZE (KiB) x 1024 - beside the layout's own count.

    python3 profiles/pmc_reduce_dia_code.py <fetch_csv> <write_csv> <timing_log> case [case ...] > summary"""
import csv
import re
import sys


def launches(path, counter):
    rows = [r for r in csv.DictReader(open(path)) if r["Counter_Name"] == counter and "k_spmv<0" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return rows


fcsv, wcsv, tlog = sys.argv[1:4]
cases = sys.argv[4:]
f, w = launches(fcsv, "FETCH_SIZE"), launches(wcsv, "WRITE_SIZE")
assert len(f) == 5 * len(cases) == len(w), (len(f), len(w), len(cases))
med = lambda a: sorted(a)[len(a) // 2]
timing = {}
for line in open(tlog):
    m = re.match(r"CASE (\S+) n=(\d+) ms=(\S+) real_bytes=(\d+)", line)
    if m:
        timing[m.group(1)] = (int(m.group(2)), float(m.group(3)), int(m.group(4)))
print(f"{'case':18s} {'states':>10s} {'us/launch':>10s} {'layout MB':>10s} {'PMC read MB':>12s} {'PMC write MB':>12s} {'PMC total MB':>12s} "
      f"{'PMC/layout':>10s} {'frac(max)':>9s}  kernel")
for i, case in enumerate(cases):
    rd = med([float(r["Counter_Value"]) for r in f[5 * i:5 * i + 5]]) * 1024.0 * 2.0
    wr = med([float(r["Counter_Value"]) for r in w[5 * i:5 * i + 5]]) * 1024.0
    n, ms, real = timing.get(case, (0, float("nan"), 0))
    tot = rd + wr
    print(f"{case:18s} {n:10d} {ms * 1e3:10.2f} {real / 1e6:10.1f} {rd / 1e6:12.1f} {wr / 1e6:12.1f} {tot / 1e6:12.1f} "
          f"{tot / max(real, 1):10.3f} {max(real, tot) / (ms * 1e-3) / 8e12:9.3f}  {f[5 * i]['Kernel_Name'][:70]}")
