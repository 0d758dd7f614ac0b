#!/bin/bash
# The measurements of profiles/local_usage/README.md in one go, from the repository root on a machine with an MI355X:
#   profiles/local_usage/measure.sh OUT [PARENT]
# OUT receives the logs; PARENT is a built checkout of the parent commit for the interleaved bench.py runs (skipped when absent).
# Every step runs under its own time limit and the script stops at the first step that fails.
set -o pipefail
O=${1:?output directory}
PARENT=$2
mkdir -p "$O"
timeout -k 10 400 python profiles/local_usage/local_usage_probe.py --tiles 512 2>&1 | tee "$O/probe.log" || exit $?
for what in usage headroom fetch; do          # one traced run per road: kernel time of the calls it makes
  timeout -k 10 180 rocprofv3 --kernel-trace --stats -d "$O/prof_$what" -o $what -f csv -- \
    python profiles/local_usage/local_usage_probe.py --no-host --only $what --scenarios 256 > "$O/traced_$what.log" 2>&1 || { echo "traced $what failed"; exit 1; }
  grep LOCAL_USAGE "$O/traced_$what.log"
done
[ -n "$PARENT" ] || exit 0
: > "$O/bench_ab.log"
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 170 python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-sub 2>/dev/null | tail -1 | sed "s/^/PARENT $i /") >> "$O/bench_ab.log" || exit $?
  (timeout -k 10 170 python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-sub 2>/dev/null | tail -1 | sed "s/^/TREE   $i /") >> "$O/bench_ab.log" || exit $?
done
grep -o '^[A-Z]* *[0-9]\|"ms_per_step": [0-9.]*' "$O/bench_ab.log" | paste - -
