#!/bin/bash
# PMC passes (FETCH_SIZE, then WRITE_SIZE + L2 hit/miss; separate runs, --kernel-trace only) over one LoRA-on UNet
# pass, summarised per kernel by scripts/pmc_summary.py; also re-runs the bench line + kernel stats.
# usage: scripts/measure_pmc.sh OUTDIR   (from the repository root)
mkdir -p "${1:?usage: scripts/measure_pmc.sh OUTDIR}"
O=$(cd "$1" && pwd)
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
python bench.py --full > $O/bench_r01.json 2> $O/bench_r01.err
tail -c 400 $O/bench_r01.err
cd /tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_bench -o bench -- python $R/bench.py --full --no-cpu-baseline > $O/prof_bench_r01.log 2>&1
find /tmp/prof_bench -name "*kernel_stats.csv" -exec cp {} $O/r01_bench_kernel_stats.csv \;
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d /tmp/pmc5 -o p -- python $R/scripts/bench_forward.py --lora --warm 0 --iters 1 > $O/t20_pmc5.log 2>&1
python $R/scripts/pmc_summary.py /tmp/pmc5 > $O/pmc_fetch_summary.csv 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d /tmp/pmc6 -o p -- python $R/scripts/bench_forward.py --lora --warm 0 --iters 1 > $O/t20_pmc6.log 2>&1
python $R/scripts/pmc_summary.py /tmp/pmc6 > $O/pmc_write_summary.csv 2>&1
cd $R; cut -c1-300 $O/bench_r01.json; tail -1 $O/prof_bench_r01.log | cut -c1-200
