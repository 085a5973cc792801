#!/bin/bash
# usage: quick_cycle.sh TAG  -- GPU parity tests, kernel trace, bench with the end-to-end leg;
# outputs under $OUT/TAG (default runs/TAG)
set -o pipefail
TAG=$1
export TMPDIR=/tmp
O=${OUT:-runs}/$TAG
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py -x -q --timeout 300 --timeout-method thread > $O/gpu.log 2>&1 || { echo TESTFAIL; tail -30 $O/gpu.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/kt -o kt --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-c5 --no-c1 --no-wire --no-e2e --steps 5 --warmup 1 > $O/kt_bench.json 2> $O/kt_bench.err || { echo KTFAIL; grep -v "^[EW]20" $O/kt_bench.err | tail; exit 2; }
timeout -k 10 300 python -u bench.py --full --steps 20 --warmup 3 --no-c5 --no-c1 --no-wire --no-cpu-baseline > $O/bench.log 2>&1 || { echo BENCHFAIL; tail $O/bench.log; exit 3; }
tail -2 $O/gpu.log
