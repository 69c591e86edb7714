#!/bin/bash
# GPU box: one rocprofv3 --pmc pass per counter set (kernel-trace only beside it) over one timed pass of the default bench.
# usage: [OUT=<dir>] [BENCH_ARGS="--workload c3"] tools/pmc_passes.sh <out-prefix> "<set 1>" "<set 2>" ...   (results under $OUT/<prefix>_<i>/)
# A pass whose counter set the hardware cannot schedule fails fast and is skipped; a timeout stops the script.
R=$(cd "$(dirname "$0")/.." && pwd)
P=$1; shift
OUT=$(mkdir -p "${OUT:-$R/out}" && cd "${OUT:-$R/out}" && pwd) && export OUT  # results: $OUT (default out/)
cd /tmp && export TMPDIR=/tmp
i=0
for SET in "$@"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $SET --kernel-trace --output-format csv -d $OUT/${P}_$i -o p -- python3 $R/bench.py --full --repeats 1 --warmup 0 --cpu-sample 0 --host-path-frames 0 $BENCH_ARGS > $OUT/${P}_$i.json 2> $OUT/${P}_$i.err
  rc=$?
  echo "pass $i rc=$rc: $SET"
  echo "$SET" > $OUT/${P}_$i.set
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "timeout: stopping"; exit 1; fi
done
exit 0
