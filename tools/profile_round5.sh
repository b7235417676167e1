#!/bin/bash
# Dev tool (GPU box): the bench lines, rocprofv3 kernel-stat summaries, per-dispatch timelines and launch censuses that profiles/r05_* hold.
# usage: bash tools/profile_round5.sh   (writes under gpurun_out/r05/)
export TMPDIR=/tmp
out=gpurun_out/r05; mkdir -p $out
python3 bench.py --full 2>/dev/null | tail -1 > $out/bench_cfg3.json
python3 bench.py --full --workload full 2>/dev/null | tail -1 > $out/bench_full.json
python3 bench.py --full --workload fullref --steps 20 --warmup 3 2>/dev/null | tail -1 > $out/bench_fullref.json
python3 bench.py --full --workload fullref --rows 4096 --steps 10 --warmup 2 2>/dev/null | tail -1 > $out/bench_fullref_rows4096.json
python3 bench.py --full --workload refdefault 2>/dev/null | tail -1 > $out/bench_refdefault.json
python3 bench.py --full --workload cfg2 2>/dev/null | tail -1 > $out/bench_cfg2.json
python3 bench.py --full --workload cfg5 2>/dev/null | tail -1 > $out/bench_cfg5.json
python3 bench.py --full --workload codeshard 2>/dev/null | tail -1 > $out/bench_codeshard.json
python3 bench.py --full --workload cfg4 2>/dev/null | tail -1 > $out/bench_cfg4.json
python3 bench.py --full --workload cfg4 --precomputed-encoders 2>/dev/null | tail -1 > $out/bench_cfg4_vq_only.json
for w in cfg3 full fullref refdefault; do
  extra=""; [ $w = full ] || [ $w = fullref ] && extra="--one-stream --no-one-stream-pass --no-half-text-pass"
  steps=2; [ $w = fullref ] && steps=6
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$w -o p -- python3 bench.py --workload $w --steps $steps --warmup 2 --cpu-rows 0 --exact-steps 0 $extra > $out/prof_$w.log 2>&1
  f=$(find $out/prof_$w -name "*kernel_stats.csv" | head -1)
  [ -n "$f" ] && head -60 "$f" | cut -c1-600 > $out/kernel_stats_$w.csv
  t=$(find $out/prof_$w -name "*kernel_trace.csv" | head -1)
  if [ -n "$t" ] && [ $w = full ]; then
    python3 tools/launch_census.py "$t" > $out/launch_census_$w.txt 2>&1
    python3 tools/timeline.py "$t" > $out/timeline_${w}_one_stream.txt 2>&1
  fi
  rm -rf $out/prof_$w
done
bash tools/r05/timeline_fullref.sh > /dev/null 2>&1; cp gpurun_out/tl/timeline.txt $out/timeline_fullref_graph_mode.txt
# PMC traffic of the headline's kernels and of the reference-shape searches', their own passes
for w in cfg3 refdefault; do
  for c in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $c --kernel-trace --output-format csv -d $out/pmc_${w}_$c -o p -- python3 bench.py --workload $w --steps 1 --warmup 1 --cpu-rows 0 --exact-steps 0 --no-clock-probe > $out/pmc_${w}_$c.log 2>&1
    f=$(find $out/pmc_${w}_$c -name "*counter_collection.csv" | head -1)
    [ -n "$f" ] && cp "$f" $out/pmc_${w}_$c.csv
    rm -rf $out/pmc_${w}_$c
  done
done
python3 tools/pmc_summary.py $out cfg3 refdefault > $out/pmc_summary.txt 2>&1
bash tools/r05/pmc_valu_refdefault.sh > /dev/null 2>&1; cp gpurun_out/valu/summary.txt $out/valu_counters_refdefault.txt
ls -la $out | head -50
