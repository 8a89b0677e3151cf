#!/bin/bash
# The assembly scan through both routes of the C++ mirror (tests/cpp/fasta_device_cli.cpp: --host = scanFastaToFiles, the file
# read, joined and cut at its N-runs on host threads; --device = scanFastaToFilesDevice, text inflated, indexed, joined and cut
# on the GPU and scanned from device memory) on one generated assembly: 1 Gb in 300 records, 80-column lines, N-gaps, telomeric
# ends; stored three ways: plain text, bgzipped (BGZF members of 65 280 bytes, zlib level 1) and plain-gzipped (one stream,
# level 1).  Flags -w 1000 -s 500 -r -g -e -i.  Per encoding: one warm-up of each route, then the two alternating three times
# with TS_TIMING=1, stdout and every output file compared every time; minimum and median of the three at the end.  Then both
# routes once with -m on the bgzipped file, and the device route once more on it under rocprofv3 --kernel-trace --stats (a run
# of its own, no counters) for the kernels' own times.  Every GPU step runs under its own time limit and ends the script when
# it fails.  Run on the GPU box.
# usage: profiles/fasta_device_rate.sh [megabases] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
MB=${1:-1000}
OUT=${2:-profiles/fasta/fasta_device_rate.txt}
TMP=${TMPDIR:-/tmp}
FA=$TMP/assembly_device_rate.fa
CLI=$TMP/fasta_device_cli
mkdir -p "$(dirname "$OUT")"
# (TS_TIMING also makes the library report every batch and call: those lines are left out of the record)
exec > >(grep --line-buffered -v -E "^ts_batch_create|^ts_scan_segments" | tee "$OUT") 2>&1
python3 - $MB "$FA" <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
mb, path = int(sys.argv[1]), sys.argv[2]
rng = np.random.default_rng(44)
n_rec = 300
w = rng.lognormal(0, 1.0, size=n_rec)
lens = np.maximum((w / w.sum() * mb * 1e6).astype(np.int64) // 80 * 80, 80 * 400)      # whole lines: the fold below is a reshape
t0 = time.time()
parts, gaps = [], 0
for i in range(n_rec):
    n = int(lens[i])
    core = seqgen.random_dna(rng, n)
    p = seqgen.mutate(rng, seqgen.repeat_array("CCCTAA", 1500), 0.02)
    q = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", 1500), 0.02)
    core[:len(p)] = p
    core[n - len(q):] = q
    for _ in range(int(rng.integers(0, 6))):
        ln = int(rng.integers(10, 5000))
        at = int(rng.integers(20000, n - 20000 - ln)) if n > 50000 + ln else 0
        if at:
            core[at:at + ln] = ord('N'); gaps += 1
    lines = np.empty((n // 80, 81), dtype=np.uint8)
    lines[:, :80] = core.reshape(-1, 80)
    lines[:, 80] = 10
    parts += [b'>scaffold_%d generated %d bp\n' % (i + 1, n), lines.tobytes()]
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
print("records %d, bases %d, gaps %d, FASTA text %.2f GB, written three ways in %.0f s" % (n_rec, int(lens.sum()), gaps, len(text) / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/fasta_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
ls -la $FA $FA.bgz $FA.gz | awk '{print $5, $9}'
WALLS=$TMP/fasta_device_walls.txt
: > $WALLS
FLAGS="-w 1000 -s 500 -r -g -e -i"
run() {     # route, tag, input, extra flags
    local t0 t1
    rm -rf $TMP/fasta_out_$1
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 300 $CLI --$1 $FLAGS $4 -o $TMP/fasta_out_$1 $3 > $TMP/fasta_stdout_$1.txt || { echo "$2 $1: failed"; exit 1; }
    t1=$(date +%s%N)
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # the two routes wrote the same bytes, or the measurement ends here
    cmp $TMP/fasta_stdout_host.txt $TMP/fasta_stdout_device.txt && diff -r $TMP/fasta_out_host $TMP/fasta_out_device > /dev/null || { echo "outputs differ"; exit 1; }
    echo "outputs equal"
}
for enc in plain bgzip gzip; do
    case $enc in plain) IN=$FA;; bgzip) IN=$FA.bgz;; gzip) IN=$FA.gz;; esac
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
echo "== with -m, bgzip"
run host "bgzipm once" $FA.bgz -m
run device "bgzipm once" $FA.bgz -m
same
du -sb $TMP/fasta_out_host $TMP/fasta_out_device | awk '{print $1, $2}'
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
    rm -rf $TMP/fasta_device_prof $TMP/fasta_out_prof
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/fasta_device_prof -o fasta_device -- $CLI --device $FLAGS -o $TMP/fasta_out_prof $FA.bgz > $TMP/fasta_stdout_prof.txt 2> $TMP/fasta_device_prof.log || { echo "the profiled run failed"; exit 1; }
    echo "== kernel stats of the device route on the bgzipped file (rocprofv3 --kernel-trace --stats):"
    find $TMP/fasta_device_prof -name '*kernel_stats.csv' | head -1 | xargs -r head -30 | sed -E 's/\([^)]*\)//' | cut -c1-200
fi
