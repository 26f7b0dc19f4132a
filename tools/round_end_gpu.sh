#!/bin/bash
# the GPU-machine half of tools/round_end.sh: bash tools/round_end_gpu.sh <tag> <git head> <covered tree hash> <source fingerprint> [tree state]
# (tree state: what ran relative to <git head>; round_end.sh runs a clean HEAD, the default)
set -uo pipefail
: "${GRAFT_REPO_ROOT:?run through gpurun}"
cd "$GRAFT_REPO_ROOT"
tag=$1; head=$2; tree=$3; fp=$4
state=${5:-HEAD, clean tree}
log=gpurun_out/${tag}_final_gpu_tests.log
mkdir -p gpurun_out
{
  echo "git_head: $head"
  echo "covered_tree_sha256: $tree"
  echo "tree_state: $state"
  echo "source_fingerprint: $fp"
  echo "date: $(date -u +%Y-%m-%dT%H:%M:%SZ)"
} > $log
# the box has no .git: what it CAN check is that the device sources it holds hash to the fingerprint the clean tree had
here=$(python -c "import bench; print(bench.source_fingerprint())")
echo "source_fingerprint_on_box: $here" >> $log
[ "$here" = "$fp" ] || { echo "round_end: RED (the box's sources are not HEAD's)" >> $log; exit 1; }
echo "---- python -m pytest tests -m gpu -x -q" >> $log
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider >> $log 2>&1
rc_tests=$?
echo "pytest_rc: $rc_tests" >> $log
[ $rc_tests -eq 0 ] || { echo "round_end: RED (pytest -m gpu)" >> $log; exit 1; }
echo "---- __graft_entry__.smoke()" >> $log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" >> $log 2>&1
rc_smoke=$?
echo "smoke_rc: $rc_smoke" >> $log
[ $rc_smoke -eq 0 ] || { echo "round_end: RED (smoke)" >> $log; exit 1; }
# the plain run as it is timed for every change: the whole process against 30 s outside its steps
echo "---- python bench.py --gpus 1 --steps 16 --warmup 2" >> $log
plain_json=${log%_gpu_tests.log}_plain_bench.json
t0=$(date +%s.%N)
timeout -k 10 300 python bench.py --gpus 1 --steps 16 --warmup 2 > "$plain_json" 2> "${plain_json%.json}.err"
rc_plain=$?
t1=$(date +%s.%N)
echo "plain_bench_rc: $rc_plain" >> $log
[ $rc_plain -eq 0 ] || { cat "${plain_json%.json}.err" >> $log; echo "round_end: RED (plain bench.py)" >> $log; exit 1; }
python - "$plain_json" "$t0" "$t1" >> $log 2>&1 <<'PY'
import json, sys
j = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
wall = float(sys.argv[3]) - float(sys.argv[2])
outside = wall - (j["steps"] + j["warmup"]) * j["ms_per_step"] / 1e3
print("plain_bench: value %.1f %s, ms_per_step %.2f, process wall %.2f s, outside the steps %.2f s" % (j["value"], j["unit"], j["ms_per_step"], wall, outside))
assert outside <= 30.0, "the plain run spends more than 30 s outside its steps"
PY
[ $? -eq 0 ] || { echo "round_end: RED (plain bench.py outside its steps)" >> $log; exit 1; }
echo "---- python bench.py --full" >> $log
bench_json=${log%_gpu_tests.log}_bench.json
timeout -k 10 900 python bench.py --full > "$bench_json" 2> "${bench_json%.json}.err"
rc_bench=$?
echo "bench_rc: $rc_bench" >> $log
[ $rc_bench -eq 0 ] || cat "${bench_json%.json}.err" >> $log   # (the runtime's stderr goes into the log only when the run failed)
python - >> $log 2>&1 <<PY
import json
j = json.loads(open("gpurun_out/${tag}_final_bench.json").read().strip().splitlines()[-1])
g = j.get("general_scene", {})
print("bench: value %.1f %s, ms_per_step %.2f, roofline.frac %.4f (%s), general_scene %.1f, fractions_refused %s" % (
    j["value"], j["unit"], j["ms_per_step"], j["roofline"]["frac"], j["roofline"]["kernel"], g.get("msamples_per_s", float("nan")), j.get("fractions_refused")))
assert "fractions_refused" not in j
PY
rc_line=$?
[ $rc_bench -eq 0 ] && [ $rc_line -eq 0 ] || { echo "round_end: RED (bench.py)" >> $log; exit 1; }
echo "round_end: GREEN at $head ($state)" >> $log
