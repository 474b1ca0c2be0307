#!/bin/bash
# The interior path of the folded banded product (option dia_code_inner) against the commit before, on one
# MI355X in one session:
#   1. python bench.py --gpus 1 --steps 200 --warmup 20, parent and this tree alternating, RUNS runs each
#      (+ --dump-outputs once per side, compared byte for byte)
#   2. interior against present path in one process, window by window (profiles/dia_inner_measure.py)
#   3. rocprofv3 --kernel-trace --stats of the bench command on both sides, each in a run of its own
#   4. counter-only rocprofv3 --pmc passes of the product on c3 - the SQ counter groups of profiles/pmc_box_sq.sh, present
#      path and interior path - each group in a run of its own
# PARENT = a checkout of the parent commit with its library built (python __graft_entry__.py), OUT = the directory the results
# go to (copied by hand to profiles/dia_inner_*).  Run from the repository root.  Every GPU step has its own time limit and
# the script ends at the first step that fails.  STEPS: which of the four parts to run (default all).
set -e
set -o pipefail
R=$PWD
P=$(cd ${PARENT:?PARENT=<checkout of the parent commit>} && pwd)
O=${OUT:?OUT=<directory for the results>}
N=${RUNS:-4}
S=${STEPS:-1234}
mkdir -p $O
O=$(cd $O && pwd)
export TMPDIR=${TMPDIR:-/tmp}
if [[ $S == *1* ]]; then
for i in $(seq 1 $N); do
  D=""; if [ $i = 1 ]; then D="--dump-outputs $O/dump_parent"; fi
  (cd $P && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $D > $O/bench_parent_$i.json 2> $O/bench_parent_$i.err)
  D=""; if [ $i = 1 ]; then D="--dump-outputs $O/dump_branch"; fi
  timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $D > $O/bench_branch_$i.json 2> $O/bench_branch_$i.err
  echo "run $i: parent $(grep -o '"ms_per_step": [0-9.]*' $O/bench_parent_$i.json) branch $(grep -o '"ms_per_step": [0-9.]*' $O/bench_branch_$i.json)"
done
if cmp $O/dump_parent/y.npy $O/dump_branch/y.npy; then echo "y.npy byte-identical"; else echo "y.npy DIFFER"; fi
sha256sum $O/dump_parent/y.npy $O/dump_branch/y.npy | tee $O/y_sha256.txt
rm -rf $O/dump_parent $O/dump_branch
fi
if [[ $S == *2* ]]; then
timeout -k 10 300 python profiles/dia_inner_measure.py $O/measure.json > $O/measure.log 2>&1
grep -E "gain" $O/measure.log | cut -c1-400
fi
if [[ $S == *3* ]]; then
(cd $P && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kp -o kp -- python bench.py --gpus 1 --steps 200 --warmup 20 > $O/bench_parent_prof.json 2> $O/bench_parent_prof.err)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kb -o kb -- python bench.py --gpus 1 --steps 200 --warmup 20 > $O/bench_branch_prof.json 2> $O/bench_branch_prof.err
cp $(find $O/prof_kp -name "kp_kernel_stats.csv" | head -1) $O/kernel_stats_parent.csv
cp $(find $O/prof_kb -name "kb_kernel_stats.csv" | head -1) $O/kernel_stats_branch.csv
grep -E "k_spmv<0|k_dia_" $O/kernel_stats_parent.csv $O/kernel_stats_branch.csv | cut -c1-260
rm -rf $O/prof_kp $O/prof_kb
fi
if [[ $S == *4* ]]; then
CASES="c3:stored_fold_present c3:stored_fold_inner"
i=0
for grp in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU" \
           "SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SMEM" \
           "SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_MISC SQ_INST_CYCLES_VMEM_RD SQ_THREAD_CYCLES_VALU SQ_INST_LEVEL_VMEM SQ_LEVEL_WAVES" \
           "GRBM_GUI_ACTIVE GRBM_COUNT"; do
  i=$((i+1))
  timeout -k 10 200 rocprofv3 --pmc $grp --output-format csv -d $O/prof_sq -o g$i -- python profiles/pmc_target.py --no-time $CASES > $O/sq_g$i.log 2>&1
  cp $(find $O/prof_sq -name "g${i}_counter_collection.csv" | head -1) $O/sq_g$i.csv
  rm -rf $O/prof_sq
done
# the product launches of a counter run in order: 5 of the first case, then 5 of the second (pmc_target.py); medians per kernel
python3 - $O <<'PY' | tee $O/pmc_sq_summary.txt
import csv, glob, sys, collections
for path in sorted(glob.glob(sys.argv[1] + "/sq_g*.csv")):
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if "k_spmv<0" in r["Kernel_Name"]:
            acc[(r["Kernel_Name"].split("(")[0], r["Counter_Name"])].append(float(r["Counter_Value"]))
    for (kn, k), v in sorted(acc.items()):
        v.sort()
        print(f"{kn:54s} {k:26s} median of {len(v)} launches: {v[len(v)//2]:.6g}")
PY
fi
