#!/bin/bash
# One round-end measurement set, per workload (c3: the headline 1M/1080p; c5:
# config 5, 8M/4K orbit): kernel stats + PMC passes with one frame in flight,
# their summary (tools/pmc_summary.py, keyed on the bench's pmc_key), then the
# bench --full line that reads the fresh counters.  Outputs under $OUT_ROOT
# (default profile_out/, which git ignores).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
set -e
export TMPDIR=/tmp
export OUT_ROOT=${OUT_ROOT:-profile_out}
O=$OUT_ROOT
mkdir -p $O
for w in ${WORKLOADS:-c3 c5}; do
  case $w in
    c3) EXTRA=""; BSTEPS=600 ;;
    c5) EXTRA="--config5"; BSTEPS=240 ;;
  esac
  NAME=$w BENCH_ARGS="--inflight 1 $EXTRA" PASSES="${PASSES:-stats fetch write sq1}" STEPS=20 bash tools/profile.sh > $O/profile_$w.log 2>&1
  python3 tools/pmc_summary.py $O/prof_$w --json $O/pmc_$w.json > $O/pmc_summary_$w.txt
  timeout -k 10 600 python3 bench.py --full $EXTRA --steps $BSTEPS --pmc-json $O/pmc_$w.json > $O/bench_$w.json.log 2>&1
  grep '"metric"' $O/bench_$w.json.log | cut -c1-300
done
