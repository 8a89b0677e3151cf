#!/bin/bash
# The record walk of the device route of --bam-subset -l 42, serial (ts_bam_chunk_walk: one wave) against the parallel index
# (ts_bam_chunk_index), through tests/cpp/bam_index_cli.cpp --walk serial|index on two inputs from the generator of
# profiles/bam_device_rate.sh (same seed): its HiFi BAM (reads of ~15 000 bases) and a short-read BAM (150 bases).  Per input:
# one warm-up of each walk, then the two alternating three times with TS_TIMING=1, the kept bytes compared every time and the
# `walk` field of the stage line collected (minimum and median of three at the end); then each walk once more on the short-read
# input under rocprofv3 --kernel-trace --stats (runs of their own, no counters) for the kernels' own times.
# Every GPU step runs under its own timeout and the script ends at the first step that fails.  Run on the GPU box.
# usage: profiles/bam_index_rate.sh [HiFi reads] [short reads] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
NL=${1:-120000}
NS=${2:-2000000}
OUT=${3:-profiles/bam/bam_index_rate.txt}
TMP=${TMPDIR:-/tmp}
CLI=$TMP/bam_index_cli
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
gen() {     # reads, mean length, sd, shortest, longest, file
python3 - "$@" <<'PY'
import numpy as np, struct, sys, zlib, time
sys.path.insert(0, '.')
from tests import seqgen
n, mean, sd, lo, hi = (int(x) for x in sys.argv[1:6])
rng = np.random.default_rng(43)
lens = np.clip(rng.normal(mean, sd, size=n), lo, hi).astype(np.int64)
pool = seqgen.random_dna(rng, int(lens.sum()))
offs = np.concatenate(([0], np.cumsum(lens)))
for i in np.flatnonzero(rng.random(n) < 0.005):
    ln = int(rng.integers(300, 8000))
    t = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", ln // 6 + 1), 0.01)[:min(ln, lens[i])]
    pool[offs[i]:offs[i] + len(t)] = t
code = np.zeros(256, dtype=np.uint8)
for ch, v in zip(b"=ACMGRSVTWYHKDBN", range(16)):
    code[ch] = v
nib = code[pool]
text = b"@HD\tVN:1.6\tSO:unknown\n"
t0 = time.time()
raw_bytes = 0
with open(sys.argv[6], 'wb') as fh:
    pend = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0))
    def flush(final=False):
        global pend
        at = 0
        while len(pend) - at >= 65280 or (final and len(pend) > at):
            piece = bytes(pend[at:at + 65280]); at += len(piece)
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            payload = co.compress(piece) + co.flush()
            fh.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
                     struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
        del pend[:at]
    tags = b"npC\x08rqf" + struct.pack("<f", 0.999)
    for i in range(n):
        s = nib[offs[i]:offs[i + 1]]
        L = len(s)
        if L & 1:
            s = np.concatenate((s, np.zeros(1, dtype=np.uint8)))
        packed = ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes()
        name = b"m64011_%d/ccs" % i
        qual = rng.integers(20, 60, size=L, dtype=np.uint8).tobytes()       # noisy qualities: compress like real ones (badly)
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + packed + qual + tags
        pend += struct.pack("<i", len(body)) + body
        raw_bytes += 4 + len(body)
        if len(pend) >= 1 << 20:
            flush()
    flush(True)
    fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
print("reads %d, bases %d, uncompressed BAM %.2f GB, written in %.0f s" % (n, int(lens.sum()), raw_bytes / 1e9, time.time() - t0))
PY
}
g++ -std=c++17 -O2 -I include tests/cpp/bam_index_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
run() {     # walk, tag, input
    local t0 t1
    t0=$(date +%s%N); TS_TIMING=1 timeout -k 10 300 $CLI --bam-subset --walk $1 -l 42 $3 > $TMP/kept_$1.bam 2> $TMP/run_$1.log || { tail -5 $TMP/run_$1.log; exit 1; }
    t1=$(date +%s%N)
    grep -E "^(bamSubsetDevice|BAM subset|bam index)" $TMP/run_$1.log
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms"
}
ab() {      # label, input
    echo "==== $1"
    run serial "$1 warm-up" $2
    run index "$1 warm-up" $2
    cmp $TMP/kept_serial.bam $TMP/kept_index.bam; echo "kept bytes equal"
    : > $TMP/walk_serial.txt; : > $TMP/walk_index.txt
    for r in 1 2 3; do
        for w in serial index; do
            run $w "$1 run $r" $2
            sed -n 's/^bamSubsetDevice ([a-z]*): context 0 of 1: .* walk \([0-9.]*\) ms.*/\1/p' $TMP/run_$w.log >> $TMP/walk_$w.txt
        done
        cmp $TMP/kept_serial.bam $TMP/kept_index.bam; echo "kept bytes equal"
    done
    for w in serial index; do
        echo "$1: walk ($w) ms, three runs: $(tr '\n' ' ' < $TMP/walk_$w.txt) minimum $(sort -n $TMP/walk_$w.txt | head -1), median $(sort -n $TMP/walk_$w.txt | sed -n 2p)"
    done
}
gen $NL 15000 3000 1000 40000 $TMP/reads_index_long.bam
ab "HiFi" $TMP/reads_index_long.bam
gen $NS 150 0 150 150 $TMP/reads_index_short.bam
ab "short reads" $TMP/reads_index_short.bam
ls -la $TMP/reads_index_long.bam $TMP/reads_index_short.bam $TMP/kept_serial.bam $TMP/kept_index.bam | awk '{print $5, $9}'
if command -v rocprofv3 > /dev/null; then
    for w in serial index; do
        rm -rf $TMP/bam_index_prof_$w
        timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/bam_index_prof_$w -o bam_index -- $CLI --bam-subset --walk $w -l 42 $TMP/reads_index_short.bam > $TMP/kept_prof.bam 2> $TMP/bam_index_prof_$w.log
        echo "kernel stats, short reads, --walk $w (rocprofv3 --kernel-trace --stats):"
        find $TMP/bam_index_prof_$w -name '*kernel_stats.csv' | head -1 | xargs -r head -8 | cut -c1-260
    done
fi
