#!/bin/bash
# The host-side refactor of the block path ("One rule, one record, two files") against the commit before, on one
# MI355X in one session:
#   1. python bench.py --gpus 1 --steps 200 --warmup 20 and profiles/block_plan.py spmm (kfsp_spmm_bench(200) at k = 4 on the
#      benchmark's generator), parent and this tree alternating, RUNS runs each (+ --dump-outputs once per side, compared
#      byte for byte)
#   2. rocprofv3 --kernel-trace --stats of profiles/block_plan.py launches on both sides, each in a run of its own, no counters
# PARENT = a checkout of the parent commit with its library built (python __graft_entry__.py) and tests/test_gpu_block_sequence.py
# copied in, OUT = the directory the results go to (bench_ab.json there is what profiles/block_plan_bench_ab.json holds).
# Run from the repository root.  Every GPU step has its own time limit and the script ends at the first step that fails.
set -e
set -o pipefail
R=$PWD
P=${PARENT:?PARENT=<checkout of the parent commit>}
O=${OUT:?OUT=<directory for the results>}
N=${RUNS:-4}
S=${STEPS:-12}
mkdir -p $O
if [[ $S == *1* ]]; then
for i in $(seq 1 $N); do
  D=""; if [ $i = 1 ]; then D="--dump-outputs $O/dump_parent"; fi
  (cd $P && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $D > $O/bench_parent_$i.json 2> $O/bench_parent_$i.err)
  D=""; if [ $i = 1 ]; then D="--dump-outputs $O/dump_branch"; fi
  timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $D > $O/bench_branch_$i.json 2> $O/bench_branch_$i.err
  timeout -k 10 120 python profiles/block_plan.py spmm --root $P > $O/spmm_parent_$i.json 2> $O/spmm_parent_$i.err
  timeout -k 10 120 python profiles/block_plan.py spmm > $O/spmm_branch_$i.json 2> $O/spmm_branch_$i.err
  echo "run $i: parent $(grep -o '"ms_per_step": [0-9.]*' $O/bench_parent_$i.json) branch $(grep -o '"ms_per_step": [0-9.]*' $O/bench_branch_$i.json)" \
       "spmm parent $(grep -o '"ms_per_product": [0-9.]*' $O/spmm_parent_$i.json) branch $(grep -o '"ms_per_product": [0-9.]*' $O/spmm_branch_$i.json)"
done
if cmp $O/dump_parent/y.npy $O/dump_branch/y.npy; then echo "y.npy byte-identical"; else echo "y.npy DIFFER"; fi
sha256sum $O/dump_parent/y.npy $O/dump_branch/y.npy | tee $O/y_sha256.txt
rm -rf $O/dump_parent $O/dump_branch
python - $O $N > $O/bench_ab.json <<'EOF'
import json, statistics, sys
O, N = sys.argv[1], int(sys.argv[2])
out = {"what": "parent and branch alternating in one session on one MI355X: bench.py --gpus 1 --steps 200 --warmup 20 (ms_per_step) and "
               "kfsp_spmm_bench(200) at k = 4 on the repressilator 171^3 stored (ms_per_product, the median of 5 windows of a process)",
       "y_npy_sha256": [l.split()[0] for l in open(O + "/y_sha256.txt")]}
for key, stem in (("ms_per_step", "bench"), ("ms_per_product", "spmm")):
    runs = {s: [json.loads(open(f"{O}/{stem}_{s}_{i}.json").read().strip().splitlines()[-1])[key] for i in range(1, N + 1)] for s in ("parent", "branch")}
    med = statistics.median(runs["branch"])
    out[key] = {"parent": runs["parent"], "branch": runs["branch"], "parent_range": [min(runs["parent"]), max(runs["parent"])],
                "branch_median": med, "branch_median_inside_parent_range": bool(min(runs["parent"]) <= med <= max(runs["parent"]))}
print(json.dumps(out))
EOF
cat $O/bench_ab.json
fi
if [[ $S == *2* ]]; then
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kp -o kp -- python profiles/block_plan.py launches --root $P > $O/launches_parent.log 2>&1
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kb -o kb -- python profiles/block_plan.py launches > $O/launches_branch.log 2>&1
cp $(find $O/prof_kp -name "kp_kernel_stats.csv" | head -1) $O/kernel_stats_parent.csv
cp $(find $O/prof_kb -name "kb_kernel_stats.csv" | head -1) $O/kernel_stats_branch.csv
rm -rf $O/prof_kp $O/prof_kb
# kernel names and calls per name, both sides
for s in parent branch; do python -c "
import csv, sys
for r in sorted(csv.DictReader(open('$O/kernel_stats_$s.csv')), key=lambda r: r['Name']): print(r['Calls'], r['Name'])" > $O/calls_$s.txt; done
if cmp $O/calls_parent.txt $O/calls_branch.txt; then echo "kernel names and calls identical: $(wc -l < $O/calls_branch.txt) kernels"; else echo "kernel names or calls DIFFER"; fi
fi
