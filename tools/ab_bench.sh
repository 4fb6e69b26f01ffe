#!/bin/bash
# Same-box A/B of builds of libmsk144hip.so (boxes of the pool differ by +-4 %, so only this counts):
#   tools/ab_bench.sh <other.so> [rounds] [dumpdir]            -> alternates bench.py between the tree's library and <other.so>
#   tools/ab_bench.sh "<a.so> <b.so> ..." [rounds] [dumpdir]   -> the tree's library and every listed one, round-robin
# dumpdir: every run also writes its decoded records (bench.py --dump-outputs) to <dumpdir>/<library>_r<round>/.
# Each run has its own time limit (AB_RUN_TIMEOUT seconds, default 240); nothing further is started after a run that was killed,
# aborted or crashed.
OTHERS=$1
N=${2:-3}
DUMP=$3
for i in $(seq 1 $N); do
  for lib in "" $OTHERS; do
    name=$(basename "${lib:-tree}" .so)
    extra=""
    [ -n "$DUMP" ] && extra="--dump-outputs $DUMP/${name}_r$i"
    MSK144HIP_LIBRARY=$lib timeout -k 10 ${AB_RUN_TIMEOUT:-240} python3 bench.py --no-cpu-baseline --steps 20 --warmup 3 --sustain-seconds 0 $extra 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('$name', round(d['ms_per_step'],3), d['stage_ms'])"
    rc=${PIPESTATUS[0]}
    if [ $rc -ne 0 ]; then echo "$name round $i: bench.py ended with status $rc, stopping"; exit $rc; fi
  done
done
