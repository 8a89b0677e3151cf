#!/bin/bash
# The assembly device routes on one context against the parent commit's, and on two contexts that share this GPU.  Inputs: the
# generated 1 Gb assembly of profiles/fasta_device_rate.sh (same generator, same seed; plain text and bgzipped) under
# -w 1000 -s 500 -r -g -e -i, with and without --device-tracks, and graph (a) of profiles/gfa_annotate_rate.py (an assembly cut
# into 60 k segments with one P line per contig) at a fifth of its size, plain text.  The contenders, each a process of its own
# under its own time limit:
#   parent   $PARENT's track_text_cli --device | --device-tracks and gfa_device_cli --device   (a built checkout of the parent
#            commit: include/, tests/cpp/ and teloscope_amd/libteloscan.so; without it the parent runs are left out and the output
#            says so)
#   one      this tree, tests/cpp/assembly_routes_multi_cli.cpp --device --devices 0     (the routes' chunk steps, in place)
#   two      this tree, --device --devices 0,0                                            (the same steps, chunks dealt to two contexts)
# and two more that CONTENDERS may name, to tell apart what a difference between `parent` and `one` comes from:
#   same     this tree's headers and library under the PARENT's programs (track_text_cli.cpp, gfa_device_cli.cpp, which this tree
#            has unchanged): the chunk steps with the parent's test program around them
#   bare     `one` without --devices: the context on the current device, as the parent's programs make theirs
# One warm-up round, then three rounds with TS_TIMING=1 (the totals line and a line per context).  The contenders alternate in
# every round, and the round's first contender moves on by one from round to round, so that none always follows the same
# neighbour and a slow spell of the box meets every contender in turn (DESIGN §4 has what a fixed order recorded).  The output
# files are compared in every round; minimum, median and spread (max - min) of the three whole-process times come at the end, with
# the verdict of the one comparison that has a condition: `one`'s median may exceed `parent`'s by no more than `parent`'s own
# spread.  Two contexts on one card share its PCIe link, its copy engines and its CUs: what `two` shows is the overlap the ring
# buys on one card and the wait for the serial section, NOT a figure for several GPUs, and no bar is set on it.
# usage: [CONTENDERS="parent one two"] profiles/assembly_routes_multi_rate.sh [megabases] [graph scale] [fasta output file] [gfa output file]
set -o pipefail
cd "$(dirname "$0")/.."
MB=${1:-1000}
SCALE=${2:-0.2}
OUT_FASTA=${3:-profiles/fasta/assembly_routes_multi_rate.txt}
OUT_GFA=${4:-profiles/gfa/assembly_routes_multi_rate.txt}
PARENT=${PARENT:-ab_old/parent}
CONTENDERS=${CONTENDERS:-parent one two}
CHUNK=${CHUNK:-268435456}
TMP=${TMPDIR:-/tmp}
FA=$TMP/assembly_multi_rate.fa
GFA=$TMP/assembly_multi_rate.gfa
CLI=$TMP/assembly_routes_multi_cli
WALLS=$TMP/assembly_routes_multi_walls.txt
FLAGS="-w 1000 -s 500 -r -g -e -i"
mkdir -p "$(dirname "$OUT_FASTA")" "$(dirname "$OUT_GFA")"

generate() {
python3 - $MB "$FA" "$GFA" $SCALE <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
sys.path.insert(0, 'profiles')
from tests import seqgen
import gfa_annotate_rate as A
mb, path, gfa, scale = int(sys.argv[1]), sys.argv[2], sys.argv[3], float(sys.argv[4])
rng = np.random.default_rng(44)                                            # the generator of profiles/fasta_device_rate.sh
n_rec = 300
w = rng.lognormal(0, 1.0, size=n_rec)
lens = np.maximum((w / w.sum() * mb * 1e6).astype(np.int64) // 80 * 80, 80 * 400)
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
print("FASTA input: records %d, bases %d, gaps %d, text %.2f GB, the largest record %.0f MB" % (n_rec, int(lens.sum()), gaps, len(text) / 1e9, lens.max() / 1e6))
A.write_graph_a(gfa, np.random.default_rng(1), scale)
import os
print("GFA input: graph (a) at scale %g, %.2f GB; all written in %.0f s" % (scale, os.path.getsize(gfa) / 1e9, time.time() - t0))
PY
}

build() {
    g++ -std=c++17 -O2 -I include tests/cpp/assembly_routes_multi_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI || return 1
    for c in track_text_cli gfa_device_cli; do
        g++ -std=c++17 -O2 -I include tests/cpp/$c.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $TMP/same_$c || return 1
    done
    if [ -f "$PARENT/teloscope_amd/libteloscan.so" ]; then
        for c in track_text_cli gfa_device_cli; do
            g++ -std=c++17 -O2 -I "$PARENT/include" "$PARENT/tests/cpp/$c.cpp" -L "$PARENT/teloscope_amd" -lteloscan \
                -Wl,-rpath,"$(cd "$PARENT/teloscope_amd" && pwd)" -pthread -lz -o $TMP/parent_$c || return 1
        done
        echo "parent: $PARENT"
    else
        PARENT=
        echo "NOT RUN: the parent commit's routes (no built checkout at ${PARENT:-ab_old/parent})"
    fi
}

step() {    # label, configuration, command...: one process under its own time limit; its wall time and its TS_TIMING lines
    local label=$1 cfg=$2 t0 t1
    shift 2
    rm -rf $TMP/amr_out_$cfg
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 300 "$@" -o $TMP/amr_out_$cfg > $TMP/amr_stdout_$cfg 2> $TMP/amr_err_$cfg || { echo "$label $cfg: FAILED"; tail -5 $TMP/amr_err_$cfg; return 1; }
    t1=$(date +%s%N)
    echo "$label $cfg: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
    grep -E "^(scanFastaToFilesDevice|annotateGfaDevice)" $TMP/amr_err_$cfg | sed "s/^/    /"
}

same() {    # the contenders of a round wrote the same files, or the measurement ends here
    local ref=$1 cfg
    shift
    for cfg in "$@"; do
        diff -r $TMP/amr_out_$ref $TMP/amr_out_$cfg > /dev/null || { echo "outputs differ: $ref against $cfg"; return 1; }
    done
    echo "outputs equal"
}

rounds() {  # tag, the parent's command, this tree's arguments...
    local tag=$1 parent=$2 r c n=0 first=0 i list=() ran
    shift 2
    for c in $CONTENDERS; do
        if [ $c = parent ] && { [ -z "$PARENT" ] || [ -z "$parent" ]; }; then continue; fi
        list+=($c)
    done
    n=${#list[@]}
    echo "== $tag"
    for r in warm-up "run 1" "run 2" "run 3"; do
        ran=
        for (( i = 0; i < n; i++ )); do
            c=${list[$(( (first + i) % n ))]}
            case $c in
                parent) step "$tag $r" parent $parent || return 1;;
                same)   step "$tag $r" same ${parent//parent_/same_} || return 1;;
                one)    step "$tag $r" one $CLI "$@" --devices 0 || return 1;;
                bare)   step "$tag $r" bare $CLI "$@" || return 1;;
                two)    step "$tag $r" two $CLI "$@" --devices 0,0 || return 1;;
                *)      echo "unknown contender $c"; return 1;;
            esac
            ran="$ran $c"
        done
        same $ran || return 1
        first=$(( first + 1 ))
    done
}

summary() {
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(.+) run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault(m.group(1), {}).setdefault(m.group(2), []).append(int(m.group(3)))
print("== minimum / median / spread (max - min) of the three runs, whole process, wall ms")
for tag, by in walls.items():
    for cfg in ("parent", "same", "one", "bare", "two"):
        if cfg in by:
            w = sorted(by[cfg])
            print("%-28s %-6s min %6d  median %6d  spread %5d" % (tag, cfg, w[0], w[len(w) // 2], w[-1] - w[0]))
    for cfg in ("one", "same", "bare"):
        if "parent" in by and cfg in by:
            p, o = sorted(by["parent"]), sorted(by[cfg])
            over = o[len(o) // 2] - p[len(p) // 2]
            print("%-28s %s's median - parent's median = %+d ms against parent's spread of %d ms: %s" %
                  (tag, cfg, over, p[-1] - p[0], "within it" if over <= p[-1] - p[0] else "EXCEEDS it: find out why before merging"))
print("`two` is two contexts on ONE card (one PCIe link, one set of copy engines and CUs): no multi-GPU rate, no bar on it.")
PY
}

measure() {     # which: fasta | gfa
    : > $WALLS
    if [ "$1" = fasta ]; then
        for enc in plain bgzip; do
            case $enc in plain) IN=$FA;; bgzip) IN=$FA.bgz;; esac
            rounds "$enc records" "$TMP/parent_track_text_cli --device $FLAGS --chunk-bytes $CHUNK $IN" --fasta --device $FLAGS --chunk-bytes $CHUNK $IN || return 1
            rounds "$enc device-tracks" "$TMP/parent_track_text_cli --device-tracks $FLAGS --chunk-bytes $CHUNK $IN" --fasta --device --device-tracks $FLAGS --chunk-bytes $CHUNK $IN || return 1
        done
    else
        # (the parent's CLI writes into the directory it is given, this tree's too: the same two files)
        rounds "graph (a) plain" "$TMP/parent_gfa_device_cli --device --chunk-bytes $CHUNK -f $GFA" --gfa --device --chunk-bytes $CHUNK $GFA || return 1
    fi
    summary
}

generate > $TMP/amr_generate.txt 2>&1 || { cat $TMP/amr_generate.txt; echo "generating the inputs failed"; exit 1; }
build > $TMP/amr_build.txt 2>&1 || { cat $TMP/amr_build.txt; echo "building the programs failed"; exit 1; }
[ -f "$PARENT/teloscope_amd/libteloscan.so" ] || PARENT=
# (TS_TIMING also makes the library report every batch and call: those lines are left out of the record)
{ grep -v "^GFA input" $TMP/amr_generate.txt; cat $TMP/amr_build.txt; measure fasta; } 2>&1 | grep --line-buffered -v -E "^ts_batch_create|^ts_scan_segments" | tee "$OUT_FASTA" || exit 1   # (a step that failed ends the measurement)
{ grep -v "^FASTA input" $TMP/amr_generate.txt; cat $TMP/amr_build.txt; measure gfa; } 2>&1 | grep --line-buffered -v -E "^ts_batch_create|^ts_scan_segments" | tee "$OUT_GFA"
