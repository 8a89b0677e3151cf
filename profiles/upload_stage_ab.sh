#!/bin/bash
# The host upload (pipeline.cpp: upload_pieces over upload_stage_core.h) of this tree against a library built from the parent
# commit: the same Python package, scripts and inputs for both, only TELOSCAN_LIB differs.  Per round and build, two processes:
#   a) profiles/stage_timing.sh's command — bench.py --full --steps 5 --warmup 2 --no-reads --no-cpu-baseline under TS_TIMING=1
#      TS_STAGE_TIMING=1: the pcie_inclusive legs of its JSON line (Gbases/s host to host, best of three calls each) and the sums of
#      the "upload_pieces:" lines on stderr (waiting for a slot, packing, runs + DMA + unpack enqueue; ms over all calls of the run)
#   b) profiles/text_in_rate.py with REPS=4: joined bases and FASTA text in, best of four calls each
# The build that goes first alternates from round to round.  At the end, per figure: the parent's runs, their median and range, the
# child's runs and median, and whether the child's median lies within the parent's range; then bench.py's default line (child).
# Run on the GPU box.   usage: profiles/upload_stage_ab.sh PARENT_LIB [rounds] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
PARENT_LIB=$(readlink -f "${1:?usage: profiles/upload_stage_ab.sh PARENT_LIB [rounds] [output file]}")
ROUNDS=${2:-5}
OUT=${3:-profiles/upload/stage_refactor_ab.txt}
CHILD_LIB=$PWD/teloscope_amd/libteloscan.so
[ -f "$PARENT_LIB" ] && [ -f "$CHILD_LIB" ]
TMP=${TMPDIR:-/tmp}/upload_stage_ab
mkdir -p $TMP "$(dirname "$OUT")"
LOG=$TMP/runs.txt
: > $LOG
one() {     # who, round: both processes with that build's library, their figures appended to the log
    local who=$1 r=$2 lib
    case $who in parent) lib=$PARENT_LIB;; child) lib=$CHILD_LIB;; esac
    TELOSCAN_LIB=$lib TS_TIMING=1 TS_STAGE_TIMING=1 timeout -k 10 400 python3 bench.py --full --steps 5 --warmup 2 --no-reads --no-cpu-baseline \
        > $TMP/bench.json 2> $TMP/bench.err || { echo "$who run $r: bench.py --full failed" | tee -a $LOG; tail -5 $TMP/bench.err; return 1; }
    python3 - $who $r $TMP/bench.json $TMP/bench.err >> $LOG <<'PY'
import json, re, sys
who, r = sys.argv[1], sys.argv[2]
d = json.loads(open(sys.argv[3]).read().strip().splitlines()[-1])
for leg, v in d["pcie_inclusive"].items():
    if isinstance(v, dict) and "gbases_per_s" in v:
        print("%s run %s: pcie_inclusive %s = %.3f Gbases/s" % (who, r, leg, v["gbases_per_s"]))
sums, lines = [0.0, 0.0, 0.0], 0
for line in open(sys.argv[4]):
    m = re.search(r"upload_pieces: (\d+) chunks, waiting for a free slot ([0-9.]+) ms, packing ([0-9.]+) ms, runs \+ DMA \+ unpack enqueue ([0-9.]+) ms", line)
    if m:
        lines += 1
        for q in range(3):
            sums[q] += float(m.group(2 + q))
for q, name in enumerate(("waiting", "packing", "issue")):
    print("%s run %s: stage_timing %s = %.2f ms over %d upload_pieces lines" % (who, r, name, sums[q], lines))
PY
    TELOSCAN_LIB=$lib REPS=4 timeout -k 10 300 python3 profiles/text_in_rate.py > $TMP/text.out 2> $TMP/text.err \
        || { echo "$who run $r: text_in_rate.py failed" | tee -a $LOG; tail -5 $TMP/text.err; return 1; }
    grep "^best of all" $TMP/text.out | sed -e "s/^best of all: *\(.*[a-z]\) *[0-9.]* ms = \([0-9.]*\) Gbases.*/$who run $r: text_in_rate \1 = \2 Gbases\/s/" -e "s/ \+/ /g" >> $LOG
    tail -12 $LOG | grep "^$who run $r:" | sed -e "s/^/  /"
}
for r in $(seq $ROUNDS); do
    if [ $((r % 2)) = 1 ]; then one parent $r && one child $r || exit 1; else one child $r && one parent $r || exit 1; fi
done
{
    echo "Parent / child record of the refactor that moved the staging of the host upload's chunks out of upload_pieces (pipeline.cpp) into"
    echo "upload_stage_core.h.  One MI355X, other people's work on the same host.  Two builds of libteloscan.so, the parent commit's and"
    echo "the child's, alternated in one session ($ROUNDS rounds, the build that goes first alternating); the same Python package, scripts and"
    echo "inputs for both (profiles/upload_stage_ab.sh).  \"Range\" is the parent's own minimum..maximum over its runs; the child's median is"
    echo "held against it.  Gbases/s: higher is better; stage_timing ms (sums over all upload_pieces calls of a run): lower is better."
    echo
    echo "================================================================ summary"
    python3 - $LOG <<'PY'
import re, sys
runs = {}
for line in open(sys.argv[1]):
    m = re.match(r"(parent|child) run \d+: (.*?) = ([0-9.]+) (\S+)", line)
    if m:
        runs.setdefault(m.group(2) + " (" + m.group(4) + ")", {}).setdefault(m.group(1), []).append(float(m.group(3)))
def median(w):
    w = sorted(w)
    return w[len(w) // 2] if len(w) % 2 else (w[len(w) // 2 - 1] + w[len(w) // 2]) / 2
for name, w in runs.items():
    p, c = w.get("parent", []), w.get("child", [])
    lo, hi, mc = min(p), max(p), median(c)
    verdict = "within the parent's range" if lo <= mc <= hi else "OUTSIDE the parent's range, %+.1f %% of its median" % (100 * (mc - median(p)) / median(p))
    print("%-62s parent %s median %.3f range %.3f..%.3f | child %s median %.3f | %s" % (name, p, median(p), lo, hi, c, mc, verdict))
PY
    echo
    echo "================================================================ the runs"
    cat $LOG
    echo
    echo "================================================================ bench.py --gpus 1 --steps 20 --warmup 5 (child; the resident scan)"
    timeout -k 10 600 python3 bench.py --gpus 1 --steps 20 --warmup 5 | tail -1
} > "$OUT"
cat "$OUT"
