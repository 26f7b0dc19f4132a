#!/bin/bash
# Round-2 profile on the GPU box (one gpurun call): the default bench line, rocprofv3 kernel traces with the passes in flight and with the
# passes serial, and the counter passes (never next to tracing): SQ x2, FETCH_SIZE, WRITE_SIZE + TCC.
# usage: bash tools/profile_round2.sh <tag> [config]      -> gpurun_out/<tag>_*
tag=${1:-r02_x}; cfg=${2:-2}
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
B="python3 $R/bench.py --full --config $cfg"
$B > $R/gpurun_out/${tag}_bench.json 2> $R/gpurun_out/${tag}_bench.err; echo "bench rc=$?"
rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/${tag}_stats -- $B --steps 4 --warmup 1 --no-cpu-baseline > $R/gpurun_out/${tag}_stats.log 2>&1
find $R/gpurun_out/${tag}_stats -name "*kernel_stats.csv" -exec cp {} $R/gpurun_out/${tag}_kernel_stats.csv \;
export FH_PIPELINE=0
$B --steps 4 --warmup 1 --no-cpu-baseline > $R/gpurun_out/${tag}_serial_bench.json 2> /dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/${tag}_serial_stats -- $B --steps 4 --warmup 1 --no-cpu-baseline > $R/gpurun_out/${tag}_serial_stats.log 2>&1
find $R/gpurun_out/${tag}_serial_stats -name "*kernel_stats.csv" -exec cp {} $R/gpurun_out/${tag}_serial_kernel_stats.csv \;
find $R/gpurun_out/${tag}_stats $R/gpurun_out/${tag}_serial_stats -name "*kernel_trace.csv" -delete
run() { name=$1; shift
  rocprofv3 --pmc "$@" --output-format csv -d $R/gpurun_out/${tag}_$name -- $B --steps 1 --warmup 1 --spp 384 --no-cpu-baseline > $R/gpurun_out/${tag}_$name.log 2>&1; echo "pmc $name rc=$?"
}
run sqa SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD
run sqb SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU SQ_INSTS_VMEM_WR GRBM_GUI_ACTIVE
run fetch FETCH_SIZE
run tcc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum
cd $R
python3 tools/pmc_summary.py "gpurun_out/${tag}_sq?/**/*counter_collection.csv" "gpurun_out/${tag}_fetch/**/*counter_collection.csv" "gpurun_out/${tag}_tcc/**/*counter_collection.csv" > gpurun_out/${tag}_pmc_summary.txt 2>&1
find gpurun_out/${tag}_sq? gpurun_out/${tag}_fetch gpurun_out/${tag}_tcc -name "*counter_collection.csv" -delete
cut -c1-700 gpurun_out/${tag}_bench.json; head -14 gpurun_out/${tag}_serial_kernel_stats.csv | cut -c1-200
