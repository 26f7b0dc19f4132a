#!/bin/bash
# Round profile on the GPU box: kernel trace + the two HBM counter passes (separate runs, as the MI355X guide prescribes).
# usage: OUT_DIR=<folder tools/collect_profile.py reads> bash tools/profile_round.sh <tag>      -> $OUT_DIR/<tag>_{stats,fetch,tcc}/, <tag>_pmc_summary.txt, <tag>_bench.json
tag=${1:-rXX}
out=$(realpath -m "${OUT_DIR:?set OUT_DIR to the folder tools/collect_profile.py reads}"); mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
B="python3 $R/bench.py --full"   # tools/collect_profile.py reads roofline, rates, kernel_ms_per_step_alone and cpu_baseline from the line; the profiled runs keep their replays
$B > $out/${tag}_bench.json 2> $out/${tag}_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_stats -- $B --steps 5 --warmup 1 --no-cpu-baseline > $out/${tag}_stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $out/${tag}_fetch -- $B --steps 2 --warmup 1 --no-cpu-baseline > $out/${tag}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $out/${tag}_tcc -- $B --steps 2 --warmup 1 --no-cpu-baseline > $out/${tag}_tcc.log 2>&1
cd $R
python3 tools/pmc_summary.py "$out/${tag}_fetch/**/*counter_collection.csv" "$out/${tag}_tcc/**/*counter_collection.csv" > $out/${tag}_pmc_summary.txt
find $out/${tag}_stats -name "*kernel_stats.csv" -exec cp {} $out/${tag}_kernel_stats.csv \;
# the raw per-dispatch traces are large; keep the summaries only
find $out/${tag}_stats -name "*kernel_trace.csv" -delete
tail -c 600 $out/${tag}_bench.json; head -12 $out/${tag}_kernel_stats.csv
