#!/bin/bash
# What interleaved pairs cost the device FASTQ route, -l 42, on the reads of profiles/fastq_device_rate.sh (same generator, same
# seed) with the names rewritten as pairs (@r<j>/1, @r<j>/2), stored as plain text and bgzipped (BGZF members of 65 280 bytes, zlib
# level 1).  Three programs in one call, per encoding one warm-up of each and then the three alternating three times with
# TS_TIMING=1:
#   paired    tests/cpp/fastq_pairs_cli.cpp --device    fastqSubsetPairedDevice of this build
#   unpaired  tests/cpp/fastq_device_cli.cpp --device   fastqSubsetDevice of this build
#   parent    tests/cpp/fastq_device_cli.cpp --device   fastqSubsetDevice of the parent commit's build
# The two unpaired programs must write the same bytes, every time.  At the end: minimum, median and spread of the three whole
# processes, and whether this build's unpaired median lies within the parent's own spread (it compiles to the same steps).  What
# pairing adds is reported, not barred.  Then the paired route once more on the bgzipped file under rocprofv3 --kernel-trace
# --stats (a run of its own, no counters) for the two new kernels' own times.  Run on the GPU box.
#
# PARENT is a tree of the parent commit with its library built, for example
#   mkdir ab_old && git archive HEAD~1 | tar -x -C ab_old && make -C ab_old/teloscope_amd/csrc
# usage: profiles/fastq_pairs_rate.sh [reads] [output file] [PARENT]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-100000}
OUT=${2:-profiles/reads/fastq_pairs_rate.txt}
PARENT=${3:-ab_old}
TMP=${TMPDIR:-/tmp}
FQ=$TMP/reads_pairs_rate.fq
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
[ -f "$PARENT/teloscope_amd/libteloscan.so" ] || { echo "no parent build at $PARENT (see the head of this script)"; exit 1; }
python3 - $N "$FQ" <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
n, path = int(sys.argv[1]) // 2 * 2, sys.argv[2]
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
parts = []
for i in range(n):
    s = buf[offs[i]:offs[i + 1]]
    parts += [b'@r%d/%d\n' % (i // 2, 1 + i % 2), s, b'\n+\n', b'I' * len(s), b'\n']
text = b"".join(parts)
del parts
open(path, 'wb').write(text)
def member(a):
    piece = text[a:a + 65280]
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    payload = co.compress(piece) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
            struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
with ThreadPoolExecutor(16) as ex, open(path + '.bgz', 'wb') as fh:          # (zlib releases the interpreter lock)
    for m in ex.map(member, range(0, len(text), 65280), chunksize=64):
        fh.write(m)
    fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
print("reads %d in %d pairs, bases %d, FASTQ text %.2f GB, written two ways in %.0f s" % (n, n // 2, int(lens.sum()), len(text) / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/fastq_pairs_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $TMP/pairs_rate_paired
g++ -std=c++17 -O2 -I include tests/cpp/fastq_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $TMP/pairs_rate_unpaired
g++ -std=c++17 -O2 -I $PARENT/include $PARENT/tests/cpp/fastq_device_cli.cpp -L $PARENT/teloscope_amd -lteloscan -Wl,-rpath,$(cd $PARENT && pwd)/teloscope_amd -pthread -lz -o $TMP/pairs_rate_parent
ls -la $FQ $FQ.bgz | awk '{print $5, $9}'
WALLS=$TMP/fastq_pairs_walls.txt
: > $WALLS
run() {     # program, tag, input: one whole process (the batch planner's lines are left out of the record)
    local t0 t1
    t0=$(date +%s%N)
    if [ $1 = paired ]; then
        TS_TIMING=1 timeout -k 10 300 $TMP/pairs_rate_paired --device -l 42 $3 2> $TMP/pairs_rate_stderr.txt > $TMP/kept_$1.fq || { tail -5 $TMP/pairs_rate_stderr.txt; exit 1; }
    else
        TS_TIMING=1 timeout -k 10 300 $TMP/pairs_rate_$1 --fastq-subset --device -l 42 $3 2> $TMP/pairs_rate_stderr.txt > $TMP/kept_$1.fq || { tail -5 $TMP/pairs_rate_stderr.txt; exit 1; }
    fi
    t1=$(date +%s%N)
    grep -v '^ts_batch_create:\|^ts_filter_reads:' $TMP/pairs_rate_stderr.txt || true
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # this build's unpaired route and the parent's wrote the same bytes, or the measurement ends here
    cmp $TMP/kept_unpaired.fq $TMP/kept_parent.fq || { echo "the unpaired bytes differ from the parent's"; exit 1; }
    echo "unpaired bytes equal the parent's"
}
for enc in plain bgzip; do
    case $enc in plain) IN=$FQ;; bgzip) IN=$FQ.bgz;; esac
    echo "== $enc"
    for p in paired unpaired parent; do run $p "$enc warm-up" $IN; done
    same
    for r in 1 2 3; do
        for p in paired unpaired parent; do run $p "$enc run $r" $IN; done
        same
    done
done
ls -la $TMP/kept_paired.fq $TMP/kept_unpaired.fq | awk '{print $5, $9}'
echo "== minimum / median / maximum of the three runs, wall ms of the whole process"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2)), []).append(int(m.group(3)))
med = lambda w: sorted(w)[len(w) // 2]
for (enc, prog), w in sorted(walls.items()):
    print("%-6s %-9s min %6d  median %6d  max %6d" % (enc, prog, min(w), med(w), max(w)))
for enc in sorted({e for e, _ in walls}):
    new, old, pair = walls[enc, "unpaired"], walls[enc, "parent"], walls[enc, "paired"]
    print("%-6s unpaired median %d ms, the parent's runs span %d .. %d ms: %s" % (enc, med(new), min(old), max(old), "within" if min(old) <= med(new) <= max(old) else
          "below" if med(new) < min(old) else "ABOVE"))
    print("%-6s pairing adds %+d ms (median against this build's unpaired median, %+.1f %%)" % (enc, med(pair) - med(new), 100.0 * (med(pair) - med(new)) / med(new)))
PY
if command -v rocprofv3 > /dev/null; then
    rm -rf $TMP/fastq_pairs_prof
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/fastq_pairs_prof -o fastq_pairs -- $TMP/pairs_rate_paired --device -l 42 $FQ.bgz > $TMP/kept_prof.fq 2> $TMP/fastq_pairs_prof.log
    echo "== kernel stats of the paired route on the bgzipped file (rocprofv3 --kernel-trace --stats): the head, and the two new kernels"
    STATS=$(find $TMP/fastq_pairs_prof -name '*kernel_stats.csv' | head -1)
    if [ -n "$STATS" ]; then head -12 $STATS | cut -c1-200; grep 'ts_fastq_mates_kernel\|ts_fastq_pair_pass_kernel' $STATS | cut -c1-200; fi
fi
rm -f $FQ $FQ.bgz $TMP/kept_paired.fq $TMP/kept_unpaired.fq $TMP/kept_parent.fq $TMP/kept_prof.fq
