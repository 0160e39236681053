#!/bin/bash
# Round 6: the whole -m gpu suite, the default bench line, and the headline-only kernel stats
set -u
OUT=${OUT:-out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 1500 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/suite_r06.log 2>&1; rc=$?
tail -4 $OUT/suite_r06.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python -u bench.py --full > $OUT/bench_r06.log 2>&1 || { tail -5 $OUT/bench_r06.log; exit 1; }
tail -c 3000 $OUT/bench_r06.log
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/benchprof_r06 -o bench -- python3 -u bench.py --full --no-extras --steps 50 --warmup 5 > $OUT/benchprof_r06.log 2>&1 || exit $?
python3 scripts/kstats.py $OUT/benchprof_r06 6 || true
