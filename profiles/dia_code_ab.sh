#!/bin/bash
# The banded product with dictionary-coded values against the commit before it, on one MI355X in one session:
#   1. python bench.py --gpus 1 --steps 200 --warmup 20, parent and this tree alternating, three runs each (+ --dump-outputs once
#      each, compared byte for byte)
#   2. rocprofv3 --kernel-trace --stats of the same command on both sides
#   3. counter-only rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the product on c3 and c3x (coded) and c3 (plain, dia_code = 0)
# PARENT = a checkout of the parent commit with its library built (python __graft_entry__.py), OUT = the directory the results
# go to (copied by hand to profiles/dia_code_*).  Run from the repository root.  Every GPU step has its own time limit and the
# script ends at the first step that fails.
set -e
R=$PWD
P=${PARENT:?PARENT=<checkout of the parent commit>}
O=${OUT:?OUT=<directory for the results>}
mkdir -p $O
for i in 1 2 3; do
  D=""; if [ $i = 1 ]; then D="--dump-outputs $O/dump_parent"; fi
  (cd $P && timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $D > $O/bench_parent_$i.json 2> $O/bench_parent_$i.err)
  D=""; if [ $i = 1 ]; then D="--dump-outputs $O/dump_branch"; fi
  timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 20 $D > $O/bench_branch_$i.json 2> $O/bench_branch_$i.err
  echo "run $i: parent $(grep -o '"ms_per_step": [0-9.]*' $O/bench_parent_$i.json) branch $(grep -o '"ms_per_step": [0-9.]*' $O/bench_branch_$i.json)"
done
if cmp $O/dump_parent/y.npy $O/dump_branch/y.npy; then echo "y.npy byte-identical"; else echo "y.npy DIFFER"; fi
(cd $P && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kp -o kp -- python bench.py --gpus 1 --steps 200 --warmup 20 > $O/bench_parent_prof.json 2> $O/bench_parent_prof.err)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kb -o kb -- python bench.py --gpus 1 --steps 200 --warmup 20 > $O/bench_branch_prof.json 2> $O/bench_branch_prof.err
cp $(find $O/prof_kp -name "kp_kernel_stats.csv" | head -1) $O/kernel_stats_parent.csv
cp $(find $O/prof_kb -name "kb_kernel_stats.csv" | head -1) $O/kernel_stats_branch.csv
grep "k_spmv<0" $O/kernel_stats_parent.csv $O/kernel_stats_branch.csv | cut -c1-260
CASES="c3:stored c3x:stored c3:stored_plain"
timeout -k 10 300 python profiles/pmc_target.py $CASES > $O/timing.log 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/prof_f -o pf -- python profiles/pmc_target.py --no-time $CASES > $O/pf.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/prof_w -o pw -- python profiles/pmc_target.py --no-time $CASES > $O/pw.log 2>&1
cp $(find $O/prof_f -name "pf_counter_collection.csv" | head -1) $O/pmc_fetch.csv
cp $(find $O/prof_w -name "pw_counter_collection.csv" | head -1) $O/pmc_write.csv
python profiles/pmc_reduce_dia_code.py $O/pmc_fetch.csv $O/pmc_write.csv $O/timing.log $CASES | tee $O/pmc_summary.txt
