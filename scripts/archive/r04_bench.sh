#!/bin/bash
# Round 4: the default bench line, its rocprofv3 kernel stats, and the config-4 traffic counters.
set -u
OUT=${OUT:-out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u bench.py --full > $OUT/bench.log 2>&1 || { tail -5 $OUT/bench.log; exit 1; }
tail -c 2500 $OUT/bench.log
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/benchprof -o bench -- python3 -u bench.py --full --steps 20 --warmup 5 > $OUT/benchprof.log 2>&1 || exit $?
bash scripts/pmc_c4.sh > $OUT/pmc_c4.log 2>&1; tail -3 $OUT/pmc_c4.log
