#!/bin/bash
# --fastq-subset -l 42 through both routes of the C++ mirror (tests/cpp/fastq_device_cli.cpp: --host = fastqSubset, lines found
# and sequences copied on the host; --device = fastqSubsetDevice, lines indexed, records framed, sequences staged and passing
# records gathered on the GPU) on the reads of profiles/fastq_subset_rate.sh (same generator, same seed), stored three ways:
# plain text, bgzipped (BGZF members of 65 280 bytes, zlib level 1) and plain-gzipped (one stream, level 1).  Per encoding: one
# warm-up of each route, then the two alternating three times with TS_TIMING=1, the kept bytes compared every time; minimum and
# median of the three at the end.  Then the device route once more on the bgzipped file under rocprofv3 --kernel-trace --stats
# (a run of its own, no counters) for the kernels' own times.  Run on the GPU box.
# usage: profiles/fastq_device_rate.sh [reads] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-100000}
OUT=${2:-profiles/fastq/fastq_device_rate.txt}
TMP=${TMPDIR:-/tmp}
FQ=$TMP/reads_device_rate.fq
CLI=$TMP/fastq_device_cli
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
python3 - $N "$FQ" <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
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
parts = []
for i in range(n):
    s = buf[offs[i]:offs[i + 1]]
    parts += [b'@r%d\n' % i, s, b'\n+\n', b'I' * len(s), b'\n']
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
co = zlib.compressobj(1, zlib.DEFLATED, 31)
with open(path + '.gz', 'wb') as fh:
    for a in range(0, len(text), 64 << 20):
        fh.write(co.compress(text[a:a + (64 << 20)]))
    fh.write(co.flush())
print("reads %d, bases %d, FASTQ text %.2f GB, written three ways in %.0f s" % (n, int(lens.sum()), len(text) / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/fastq_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
ls -la $FQ $FQ.bgz $FQ.gz | awk '{print $5, $9}'
WALLS=$TMP/fastq_device_walls.txt
: > $WALLS
run() {     # route, tag, input
    local t0 t1
    t0=$(date +%s%N); TS_TIMING=1 timeout -k 10 300 $CLI --fastq-subset --$1 -l 42 $3 > $TMP/kept_$1.fq; t1=$(date +%s%N)
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # the two routes kept the same bytes, or the measurement ends here
    cmp $TMP/kept_host.fq $TMP/kept_device.fq || { echo "kept bytes differ"; exit 1; }
    echo "kept bytes equal"
}
for enc in plain bgzip gzip; do
    case $enc in plain) IN=$FQ;; bgzip) IN=$FQ.bgz;; gzip) IN=$FQ.gz;; esac
    echo "== $enc"
    run host "$enc warm-up" $IN
    run device "$enc warm-up" $IN
    same
    for r in 1 2 3; do
        run host "$enc run $r" $IN
        run device "$enc run $r" $IN
        same
    done
done
ls -la $TMP/kept_host.fq $TMP/kept_device.fq | awk '{print $5, $9}'
echo "== minimum / median of the three runs, wall ms"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2)), []).append(int(m.group(3)))
for (enc, route), w in sorted(walls.items()):
    print("%-6s %-6s min %6d  median %6d" % (enc, route, min(w), sorted(w)[len(w) // 2]))
PY
if command -v rocprofv3 > /dev/null; then
    rm -rf $TMP/fastq_device_prof
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/fastq_device_prof -o fastq_device -- $CLI --fastq-subset --device -l 42 $FQ.bgz > $TMP/kept_prof.fq 2> $TMP/fastq_device_prof.log
    echo "== kernel stats of the device route on the bgzipped file (rocprofv3 --kernel-trace --stats):"
    find $TMP/fastq_device_prof -name '*kernel_stats.csv' | head -1 | xargs -r head -16 | cut -c1-200
fi
