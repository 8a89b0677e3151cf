#!/bin/bash
# --fastq-subset -p TTAGGG,TTAGG (a mixed-length set: the general kernels) through both routes of the C++ mirror
# (tests/cpp/fastq_device_cli.cpp: --host = fastqSubset -> ts_filter_reads, the general path's groups with the blocks downloaded
# and SegmentData assembled per read; --device = fastqSubsetDevice -> a general tips batch per chunk, the read predicate on the
# device) on the reads of profiles/fastq_device_rate.sh (same generator, same seed), as plain text.  One warm-up of each route,
# then the two alternating three times, the kept bytes compared every time; minimum and median of the three at the end, and the
# device route's stage times (TS_TIMING=1) from a run of their own.  Every GPU step runs under its own time limit and the steps
# are chained: the first that fails ends the script.  Run on the GPU box.
# usage: profiles/read_general_rate.sh [reads] [output file]
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-100000}
OUT=${2:-profiles/reads/read_general_rate.txt}
TMP=${TMPDIR:-/tmp}
FQ=$TMP/reads_general_rate.fq
CLI=$TMP/fastq_device_cli
SET="-p TTAGGG,TTAGG"
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
python3 - $N "$FQ" <<'PY' || exit 1
import numpy as np, sys, time
sys.path.insert(0, '.')
from tests import seqgen
n, path = int(sys.argv[1]), sys.argv[2]
rng = np.random.default_rng(43)
lens = np.clip(rng.normal(15000, 3000, size=n), 1000, 40000).astype(np.int64)
pool = seqgen.random_dna(rng, int(lens.sum()))
offs = np.concatenate(([0], np.cumsum(lens)))
for i in np.flatnonzero(rng.random(n) < 0.005):
    ln = int(rng.integers(300, 8000))
    t = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", ln // 6 + 1), 0.01)[:min(ln, lens[i])]
    pool[offs[i]:offs[i] + len(t)] = t
buf = pool.tobytes()
t0 = time.time()
with open(path, 'wb') as fh:
    for i in range(n):
        s = buf[offs[i]:offs[i + 1]]
        fh.write(b'@r%d\n' % i + s + b'\n+\n' + b'I' * len(s) + b'\n')
print("reads %d, bases %d, written as plain FASTQ text in %.0f s" % (n, int(lens.sum()), time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/fastq_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI || exit 1
ls -la $FQ | awk '{print $5, $9}'
echo "pattern set: $SET"
WALLS=$TMP/read_general_walls.txt
: > $WALLS
run() {     # route, tag: one bounded GPU step
    local t0 t1 rc
    t0=$(date +%s%N); timeout -k 10 300 $CLI --fastq-subset --$1 $SET $FQ > $TMP/kept_general_$1.fq; rc=$?; t1=$(date +%s%N)
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms (rc $rc)" | tee -a $WALLS
    return $rc
}
same() {    # the two routes kept the same bytes, or the measurement ends here
    cmp $TMP/kept_general_host.fq $TMP/kept_general_device.fq && echo "kept bytes equal"
}
run host "warm-up" && run device "warm-up" && same &&
run host "run 1" && run device "run 1" && same &&
run host "run 2" && run device "run 2" && same &&
run host "run 3" && run device "run 3" && same &&
TS_TIMING=1 timeout -k 10 300 $CLI --fastq-subset --device $SET $FQ 2>&1 > /dev/null | grep -E "fastqSubsetDevice|kept" || { echo "a step failed: the measurement ends here"; exit 1; }
ls -la $TMP/kept_general_host.fq | awk '{print $5, "bytes kept"}'
echo "== minimum / median of the three runs, wall ms (whole process)"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault(m.group(1), []).append(int(m.group(2)))
for route, w in sorted(walls.items()):
    print("%-6s min %6d  median %6d" % (route, min(w), sorted(w)[len(w) // 2]))
PY
