#!/bin/bash
# round 6: the whole GPU suite (one process), then the default bench line
set -o pipefail
mkdir -p gpurun_out
timeout -k 10 1500 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread > gpurun_out/gputests.log 2>&1 || exit $?
BENCH_OUT=${BENCH_OUT:-bench_out}; mkdir -p "$BENCH_OUT"
timeout -k 10 600 python bench.py --full > "$BENCH_OUT/bench.json" 2> "$BENCH_OUT/bench.err"
