#!/bin/bash
# The tiled scan's host plan out of tiled_plan_core.h (this tree) against a library built from the parent commit: the same Python
# package, scripts and inputs for both, only TELOSCAN_LIB differs; the device code of both builds is the same.  Per round, the
# parent first and then the child, each with two processes:
#   a) bench.py --full --no-reads --no-cpu-baseline --no-e2e --steps 20 --warmup 5: the scan kernel's ms (roofline.kernel_ms),
#      ms_per_step, scan_plus_block_calling (the step, the emitting scan alone, block calling + pack alone) and the launch_protocol
#      figures (ts_batch_create and ts_batch_sync are on their path)
#   b) bench.py --reads --steps 10 --warmup 3: ms_per_step of the read filter
# Every step under a time limit of its own; the first failure ends the script.  At the end, per figure: the parent's runs, their
# median and minimum..maximum, the child's runs and median, and whether the child's median lies within the parent's range.
# Run on the GPU box.   usage: profiles/tiled_plan_ab.sh PARENT_LIB [rounds] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
PARENT_LIB=$(readlink -f "${1:?usage: profiles/tiled_plan_ab.sh PARENT_LIB [rounds] [output file]}")
ROUNDS=${2:-4}
OUT=${3:-profiles/tiled/plan_refactor_ab.txt}
CHILD_LIB=$PWD/teloscope_amd/libteloscan.so
[ -f "$PARENT_LIB" ] && [ -f "$CHILD_LIB" ]
TMP=${TMPDIR:-/tmp}/tiled_plan_ab
mkdir -p $TMP "$(dirname "$OUT")"
LOG=$TMP/runs.txt
: > $LOG
one() {     # who, round
    local who=$1 r=$2 lib
    case $who in parent) lib=$PARENT_LIB;; child) lib=$CHILD_LIB;; esac
    TELOSCAN_LIB=$lib timeout -k 10 300 python3 bench.py --gpus 1 --full --no-reads --no-cpu-baseline --no-e2e --steps 20 --warmup 5 \
        > $TMP/bench.json 2> $TMP/bench.err || { echo "$who run $r: bench.py --full failed" | tee -a $LOG; tail -5 $TMP/bench.err; return 1; }
    TELOSCAN_LIB=$lib timeout -k 10 300 python3 bench.py --gpus 1 --reads --steps 10 --warmup 3 \
        > $TMP/reads.json 2> $TMP/reads.err || { echo "$who run $r: bench.py --reads failed" | tee -a $LOG; tail -5 $TMP/reads.err; return 1; }
    python3 - $who $r $TMP/bench.json $TMP/reads.json >> $LOG <<'PY'
import json, sys
who, r = sys.argv[1], sys.argv[2]
d = json.loads(open(sys.argv[3]).read().strip().splitlines()[-1])
figs = [("scan kernel_ms", d["roofline"]["kernel_ms"]), ("scan ms_per_step", d["ms_per_step"])]
b = d.get("scan_plus_block_calling", {})
figs += [("scan_plus_block_calling " + k, b[k]) for k in ("ms_per_step", "emitting_scan_alone_ms", "block_calling_and_pack_alone_ms") if k in b]
figs += [("launch_protocol " + k, v) for k, v in d["config"].get("launch_protocol", {}).items() if isinstance(v, (int, float))]
figs += [("reads ms_per_step", json.loads(open(sys.argv[4]).read().strip().splitlines()[-1])["ms_per_step"])]
for name, v in figs:
    print("%s run %s: %s = %.4f ms" % (who, r, name, v))
PY
    grep "^$who run $r:" $LOG | sed -e "s/^/  /"
}
for r in $(seq $ROUNDS); do
    one parent $r && one child $r || exit 1
done
{
    echo "Parent / child record of the refactor that moved the tiled scan's host plan out of capi.cpp and shard.cpp into"
    echo "tiled_plan_core.h and the kernel's LDS layout into scan_lds_core.h.  One MI355X, other people's work on the same host.  Two"
    echo "builds of libteloscan.so, the parent commit's and the child's, alternated in one session ($ROUNDS rounds, the parent first in"
    echo "every pair); the same Python package, scripts and inputs for both (profiles/tiled_plan_ab.sh).  \"Range\" is the parent's own"
    echo "minimum..maximum over its runs; the child's median is held against it.  All figures in ms: lower is better."
    echo
    echo "================================================================ summary"
    python3 - $LOG <<'PY'
import re, sys
runs = {}
for line in open(sys.argv[1]):
    m = re.match(r"(parent|child) run \d+: (.*?) = ([0-9.]+) ms", line)
    if m:
        runs.setdefault(m.group(2), {}).setdefault(m.group(1), []).append(float(m.group(3)))
def median(w):
    w = sorted(w)
    return w[len(w) // 2] if len(w) % 2 else (w[len(w) // 2 - 1] + w[len(w) // 2]) / 2
for name, w in runs.items():
    p, c = w.get("parent", []), w.get("child", [])
    lo, hi, mc = min(p), max(p), median(c)
    verdict = "within the parent's range" if lo <= mc <= hi else "OUTSIDE the parent's range, %+.1f %% of its median" % (100 * (mc - median(p)) / median(p))
    print("%-72s parent %s median %.4f range %.4f..%.4f | child %s median %.4f | %s" % (name, p, median(p), lo, hi, c, mc, verdict))
PY
    echo
    echo "================================================================ the runs"
    cat $LOG
} > "$OUT"
cat "$OUT"
