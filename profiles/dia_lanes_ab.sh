#!/bin/bash
# The lane path of the folded banded product and the fold as the default (options dia_code_lanes / dia_code_diag)
# against the commit before, on one MI355X in one session:
#   1. python bench.py --gpus 1 --steps 200 --warmup 20, parent and this tree alternating, RUNS runs each
#      (+ --dump-outputs once per side, compared byte for byte)
#   2. lanes against loads in one process, window by window (profiles/dia_lanes_measure.py)
#   3. rocprofv3 --kernel-trace --stats of the bench command on both sides
#   4. counter-only rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the product on c3 and c3x - DIAG as a stream, folded, folded
#      with the lanes - each counter in a run of its own
# PARENT = a checkout of the parent commit with its library built (python __graft_entry__.py), OUT = the directory the results
# go to (copied by hand to profiles/dia_lanes_*).  Run from the repository root.  Every GPU step has its own time limit and
# the script ends at the first step that fails.  STEPS: which of the four parts to run (default all).
set -e
set -o pipefail
R=$PWD
P=${PARENT:?PARENT=<checkout of the parent commit>}
O=${OUT:?OUT=<directory for the results>}
N=${RUNS:-4}
S=${STEPS:-1234}
mkdir -p $O
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
timeout -k 10 300 python profiles/dia_lanes_measure.py $O/measure.json > $O/measure.log 2>&1
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
CASES="c3:stored_stream c3x:stored_stream c3:stored c3x:stored c3:stored_fold_lanes c3x:stored_fold_lanes"
timeout -k 10 300 python profiles/pmc_target.py $CASES > $O/timing.log 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/prof_f -o pf -- python profiles/pmc_target.py --no-time $CASES > $O/pf.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/prof_w -o pw -- python profiles/pmc_target.py --no-time $CASES > $O/pw.log 2>&1
cp $(find $O/prof_f -name "pf_counter_collection.csv" | head -1) $O/pmc_fetch.csv
cp $(find $O/prof_w -name "pw_counter_collection.csv" | head -1) $O/pmc_write.csv
rm -rf $O/prof_f $O/prof_w
python profiles/pmc_reduce_dia_code.py $O/pmc_fetch.csv $O/pmc_write.csv $O/timing.log $CASES | tee $O/pmc_summary.txt
fi
