#!/bin/bash
# The write stage of the assembly scan, three ways, through tests/cpp/track_text_cli.cpp on the generated assembly of
# profiles/fasta_device_rate.sh (1 Gb in 300 records, 80-column lines, N-gaps, telomeric ends; plain text and bgzipped):
#   --host           scanFastaToFiles: read, joined and cut on host threads, window lines formatted by BedWriter's threads;
#   --device         scanFastaToFilesDevice: front end on the GPU, window records downloaded, the same host formatting;
#   --device-tracks  the same with deviceTracks = true: the five window tracks formatted on the GPU (tracks.hip), text downloaded.
# Flags -w 1000 -s 500 -r -g -e.  Per encoding: one warm-up of each route, then the three alternating three times with
# TS_TIMING=1 (the stage lines of every run are kept), stdout and every output file compared with the host route's every time;
# minimum and median of the three whole-process times at the end.  The yardstick of --device-tracks is --device of the same
# binary (and its "write" stage line), never itself.  Then --device-tracks once more on the bgzipped file under
# rocprofv3 --kernel-trace --stats (a run of its own, no counters) for the kernels' own times.  Every GPU step runs under its
# own time limit and ends the script when it fails.  Run on the GPU box.
# usage: profiles/track_text_rate.sh [megabases] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
MB=${1:-1000}
OUT=${2:-profiles/tracks/track_text_rate.txt}
TMP=${TMPDIR:-/tmp}
FA=$TMP/assembly_track_rate.fa
CLI=$TMP/track_text_cli
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
print("records %d, bases %d, gaps %d, FASTA text %.2f GB, written two ways in %.0f s" % (n_rec, int(lens.sum()), gaps, len(text) / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/track_text_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
ls -la $FA $FA.bgz | awk '{print $5, $9}'
WALLS=$TMP/track_text_walls.txt
: > $WALLS
FLAGS="-w 1000 -s 500 -r -g -e"
run() {     # route, tag, input
    local t0 t1
    rm -rf $TMP/track_out_$1
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 300 $CLI --$1 $FLAGS -o $TMP/track_out_$1 $3 > $TMP/track_stdout_$1.txt || { echo "$2 $1: failed"; exit 1; }
    t1=$(date +%s%N)
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # route: it wrote the bytes the host route wrote, or the measurement ends here
    cmp $TMP/track_stdout_host.txt $TMP/track_stdout_$1.txt && diff -r $TMP/track_out_host $TMP/track_out_$1 > /dev/null || { echo "outputs of $1 differ"; exit 1; }
    echo "outputs of $1 equal the host route's"
}
for enc in plain bgzip; do
    case $enc in plain) IN=$FA;; bgzip) IN=$FA.bgz;; esac
    echo "== $enc"
    run host "$enc warm-up" $IN
    run device "$enc warm-up" $IN
    same device
    run device-tracks "$enc warm-up" $IN
    same device-tracks
    for r in 1 2 3; do
        run host "$enc run $r" $IN
        run device "$enc run $r" $IN
        same device
        run device-tracks "$enc run $r" $IN
        same device-tracks
    done
done
du -sb $TMP/track_out_host $TMP/track_out_device-tracks | awk '{print $1, $2}'
echo "== minimum / median of the three runs, wall ms"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) run \d ([\w-]+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2)), []).append(int(m.group(3)))
for (enc, route), w in sorted(walls.items()):
    print("%-6s %-13s min %6d  median %6d" % (enc, route, min(w), sorted(w)[len(w) // 2]))
PY
if command -v rocprofv3 > /dev/null; then
    rm -rf $TMP/track_text_prof $TMP/track_out_prof
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/track_text_prof -o track_text -- $CLI --device-tracks $FLAGS -o $TMP/track_out_prof $FA.bgz > $TMP/track_stdout_prof.txt 2> $TMP/track_text_prof.log || { echo "the profiled run failed"; exit 1; }
    echo "== kernel stats of --device-tracks on the bgzipped file (rocprofv3 --kernel-trace --stats):"
    find $TMP/track_text_prof -name '*kernel_stats.csv' | head -1 | xargs -r head -30 | sed -E 's/\([^)]*\)//' | cut -c1-200
fi
