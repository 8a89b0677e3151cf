#!/bin/bash
# Assembly record filters through both routes of the C++ mirror (tests/cpp/assembly_device_cli.cpp: --host = the selection
# resolved on the host — FastaGroupReader(strict) + scanFastaToFiles, validateFilteredGfa + readGfa + annotateGfa; --device =
# scanFastaToFilesDevice / annotateGfaDevice with the selector, the text checked and selected from where it lies in device
# memory) on two generated inputs:
#   fasta  the assembly of profiles/fasta_device_rate.sh (1 Gb in 300 records, 80-column lines, N-gaps, telomeric ends), every
#          tenth record selected through --include-bed (30 of 300); flags -w 1000 -s 500 -r -g -e -i
#   gfa    graph (a) of profiles/gfa_annotate_rate.py (an assembly cut into 60 k segments, one P line per contig, 3 Gb at scale
#          1), a tenth of its 24 paths selected through --include-prefix ctg7,ctg13 (2 of 24); flags -x 0 -l 60
# each stored three ways: plain text, bgzipped (BGZF members of 65 280 bytes, zlib level 1) and plain-gzipped (one stream, level
# 1).  Per input and encoding: one warm-up of each route, then the two alternating three times in this one call with
# TS_TIMING=1, every output file (and the FASTA console text) compared every time; minimum and median of the three at the end.
# No bar is set on these numbers and no default depends on them: the file records what was run, at which sizes, and what was
# not.  Every GPU step runs under its own time limit and ends the script when it fails.  Run on the GPU box.
# usage: profiles/filter_device_rate.sh [fasta megabases, 0 = skip] [graph scale, 0 = skip] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
MB=${1:-1000}
SCALE=${2:-1.0}
OUT=${3:-profiles/filter/filter_device_rate.txt}
TMP=${TMPDIR:-/tmp}
FA=$TMP/filter_rate_assembly.fa
GFA=$TMP/filter_rate_graph.gfa
CLI=$TMP/assembly_device_cli
mkdir -p "$(dirname "$OUT")"
# (TS_TIMING also makes the library report every batch and call: those lines are left out of the record)
exec > >(grep --line-buffered -v -E "^ts_batch_create|^ts_scan_segments|^ts_terminal_ends" | tee "$OUT") 2>&1
echo "filter_device_rate: fasta ${MB} Mb (0 = not run), graph scale ${SCALE} (0 = not run; 1 = 3 Gb, 60 k segments)"
g++ -std=c++17 -O2 -I include tests/cpp/assembly_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
WALLS=$TMP/filter_rate_walls.txt
: > $WALLS

# the three encodings of a text file: itself, <file>.bgz and <file>.gz  (a GFA input keeps a name that ends in .gfa.gz)
encode() {  # plain file, bgzip file, gzip file
    python3 - "$1" "$2" "$3" <<'PY'
import struct, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
plain, bgz, gz = sys.argv[1:4]
t0 = time.time()
text = open(plain, 'rb').read()
def member(a):
    piece = text[a:a + 65280]
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    payload = co.compress(piece) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
            struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
with ThreadPoolExecutor(16) as ex, open(bgz, 'wb') as fh:                     # (zlib releases the interpreter lock)
    for m in ex.map(member, range(0, len(text), 65280), chunksize=64):
        fh.write(m)
    fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
co = zlib.compressobj(1, zlib.DEFLATED, 31)
with open(gz, 'wb') as fh:
    for a in range(0, len(text), 64 << 20):
        fh.write(co.compress(text[a:a + (64 << 20)]))
    fh.write(co.flush())
print("text %.2f GB, bgzipped and gzipped in %.0f s" % (len(text) / 1e9, time.time() - t0))
PY
}
run() {     # kind, route, tag, input, flags
    local t0 t1
    rm -rf $TMP/filter_out_$2
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 600 $CLI --$2 $4 $5 -o $TMP/filter_out_$2 > $TMP/filter_stdout_$2.txt || { echo "$1 $3 $2: failed"; exit 1; }
    t1=$(date +%s%N)
    echo "$1 $3 $2: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # kind: the two routes wrote the same bytes, or the measurement ends here (the GFA stats line holds times: files only)
    if [ "$1" = fasta ]; then cmp $TMP/filter_stdout_host.txt $TMP/filter_stdout_device.txt || { echo "console text differs"; exit 1; }; fi
    diff -r $TMP/filter_out_host $TMP/filter_out_device > /dev/null || { echo "outputs differ"; exit 1; }
    echo "outputs equal"
}
measure() { # kind, plain, bgzip, gzip, flags
    for enc in plain bgzip gzip; do
        case $enc in plain) IN=$2;; bgzip) IN=$3;; gzip) IN=$4;; esac
        echo "== $1 $enc"
        run $1 host "$enc warm-up" $IN "$5"
        run $1 device "$enc warm-up" $IN "$5"
        same $1
        for r in 1 2 3; do
            run $1 host "$enc run $r" $IN "$5"
            run $1 device "$enc run $r" $IN "$5"
            same $1
        done
    done
}

if [ "$MB" != 0 ]; then
    python3 - $MB "$FA" <<'PY'
import numpy as np, sys, time
sys.path.insert(0, '.')
from tests import seqgen
mb, path = int(sys.argv[1]), sys.argv[2]
rng = np.random.default_rng(44)
n_rec = 300
w = rng.lognormal(0, 1.0, size=n_rec)
lens = np.maximum((w / w.sum() * mb * 1e6).astype(np.int64) // 80 * 80, 80 * 400)      # whole lines: the fold below is a reshape
t0 = time.time()
gaps = 0
with open(path, 'wb') as fh, open(path + '.ids', 'w') as ids:
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
        fh.write(b'>scaffold_%d generated %d bp\n' % (i + 1, n))
        fh.write(lines.tobytes())
        if (i + 1) % 10 == 0:
            ids.write('scaffold_%d\n' % (i + 1))
kept = int(lens[9::10].sum())
print("fasta: records %d, bases %d, gaps %d, selected 30 records with %d bases, written in %.0f s" % (n_rec, int(lens.sum()), gaps, kept, time.time() - t0))
PY
    encode $FA $FA.bgz $FA.gz
    ls -la $FA $FA.bgz $FA.gz | awk '{print $5, $9}'
    measure fasta $FA $FA.bgz $FA.gz "-w 1000 -s 500 -r -g -e -i --include-bed $FA.ids"
else
    echo "fasta: not run"
fi

if [ "$SCALE" != 0 ]; then
    python3 - $SCALE "$GFA" <<'PY'
import sys, time
import numpy as np
sys.path.insert(0, '.')
sys.path.insert(0, 'profiles')
import gfa_annotate_rate as A
t0 = time.time()
A.write_graph_a(sys.argv[2], np.random.default_rng(1), float(sys.argv[1]))
print("gfa: graph (a) at scale %s written in %.0f s" % (sys.argv[1], time.time() - t0))
PY
    encode $GFA $GFA.bgz.gfa.gz $GFA.gz
    ls -la $GFA $GFA.bgz.gfa.gz $GFA.gz | awk '{print $5, $9}'
    measure gfa $GFA $GFA.bgz.gfa.gz $GFA.gz "-x 0 -l 60 --include-prefix ctg7,ctg13"
else
    echo "gfa: not run"
fi

echo "== minimum / median of the three runs, wall ms"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) (\w+) run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2), m.group(3)), []).append(int(m.group(4)))
for (kind, enc, route), w in sorted(walls.items()):
    print("%-6s %-6s %-6s min %6d  median %6d" % (kind, enc, route, min(w), sorted(w)[len(w) // 2]))
PY
rm -f $FA $FA.bgz $FA.gz $FA.ids $GFA $GFA.bgz.gfa.gz $GFA.gz
