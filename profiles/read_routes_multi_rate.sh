#!/bin/bash
# The device read routes on one context against the parent commit's, and on two contexts that share this GPU, on the inputs of
# profiles/fastq_device_rate.sh (plain and bgzipped FASTQ) and profiles/bam_device_rate.sh (same generators, same seed).  Three
# configurations alternate in every round, each a process of its own under its own time limit:
#   parent   $PARENT's fastq_device_cli / bam_device_cli --device   (a built checkout of the parent commit: include/, tests/cpp/
#            and teloscope_amd/libteloscan.so; without it the parent runs are left out and the output says so)
#   one      this tree, tests/cpp/read_routes_multi_cli.cpp --device --devices 0     (the routes' chunk steps, every chunk in place)
#   two      this tree, --device --devices 0,0                                        (the same steps, chunks dealt to two contexts)
# One warm-up of each, then three rounds with TS_TIMING=1 (a line per context and the write line), the kept bytes of the three
# compared in every round; minimum and median of the three at the end.  `one` must lie within the spread of `parent`, stage by
# stage: in place it does what the parent's loop did.  TELOMERIC (default 0.005) is the fraction of reads that get a telomeric
# stretch; at 1 every read passes, the bytes written are as large as the chunks, and a stray host copy of them would show in the
# gather and write figures.  Two contexts on one card share its PCIe link, its copy engines and its CUs: what they show is
# the overlap the ring buys on one card and the carry wait, not a figure for several GPUs.  Then `two` once more on the bgzipped
# FASTQ under rocprofv3 --kernel-trace --memory-copy-trace --stats (a run of its own, no counters): the commit's copy is a
# device-to-device copy, not a kernel.  Run on the GPU box.
# usage: profiles/read_routes_multi_rate.sh [fastq reads] [bam reads] [output file]
set -o pipefail
cd "$(dirname "$0")/.."
NFQ=${1:-100000}
NBAM=${2:-120000}
OUT=${3:-profiles/reads/read_routes_multi_rate.txt}
PARENT=${PARENT:-ab_old/parent}
CHUNK=${CHUNK:-268435456}
TELOMERIC=${TELOMERIC:-0.005}
TMP=${TMPDIR:-/tmp}
FQ=$TMP/reads_multi_rate.fq
BAM=$TMP/reads_multi_rate.bam
CLI=$TMP/read_routes_multi_cli
WALLS=$TMP/read_routes_multi_walls.txt
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1

generate() {
python3 - $NFQ $NBAM "$FQ" "$BAM" $TELOMERIC <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
def member(piece):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    payload = co.compress(piece) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
            struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
def bgzip(data, path):
    with ThreadPoolExecutor(16) as ex, open(path, 'wb') as fh:              # (zlib releases the interpreter lock)
        for m in ex.map(lambda a: member(data[a:a + 65280]), range(0, len(data), 65280), chunksize=64):
            fh.write(m)
        fh.write(EOF)
def reads(n):                                                               # the generator of the two rate scripts, seed 43
    rng = np.random.default_rng(43)
    lens = np.clip(rng.normal(15000, 3000, size=n), 1000, 40000).astype(np.int64)
    pool = seqgen.random_dna(rng, int(lens.sum()))
    offs = np.concatenate(([0], np.cumsum(lens)))
    for i in np.flatnonzero(rng.random(n) < float(sys.argv[5])):
        ln = int(rng.integers(300, 8000))
        t = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", ln // 6 + 1), 0.01)[:min(ln, lens[i])]
        pool[offs[i]:offs[i] + len(t)] = t
    return rng, lens, pool, offs
nfq, nbam, fq, bam = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
t0 = time.time()
rng, lens, pool, offs = reads(nfq)
buf = pool.tobytes()
parts = []
for i in range(nfq):
    s = buf[offs[i]:offs[i + 1]]
    parts += [b'@r%d\n' % i, s, b'\n+\n', b'I' * len(s), b'\n']
text = b"".join(parts)
del parts
open(fq, 'wb').write(text)
bgzip(text, fq + '.bgz')
print("FASTQ: reads %d, bases %d, text %.2f GB" % (nfq, int(lens.sum()), len(text) / 1e9))
rng, lens, pool, offs = reads(nbam)
code = np.zeros(256, dtype=np.uint8)
for ch, v in zip(b"=ACMGRSVTWYHKDBN", range(16)):
    code[ch] = v
nib = code[pool]
head = b"@HD\tVN:1.6\tSO:unknown\n"
out = [b"BAM\1" + struct.pack("<i", len(head)) + head + struct.pack("<i", 0)]
for i in range(nbam):
    s = nib[offs[i]:offs[i + 1]]
    L = len(s)
    if L & 1:
        s = np.concatenate((s, np.zeros(1, dtype=np.uint8)))
    packed = ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes()
    name = b"m64011_%d/ccs" % i
    qual = rng.integers(20, 60, size=L, dtype=np.uint8).tobytes()           # noisy qualities: compress like real ones (badly)
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + packed + qual + \
        b"npC\x08rqf" + struct.pack("<f", 0.999)
    out.append(struct.pack("<i", len(body)) + body)
raw = b"".join(out)
del out
bgzip(raw, bam)
print("BAM: reads %d, bases %d, uncompressed %.2f GB; both written in %.0f s" % (nbam, int(lens.sum()), len(raw) / 1e9, time.time() - t0))
PY
}

build() {
    g++ -std=c++17 -O2 -I include tests/cpp/read_routes_multi_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI || return 1
    if [ -f "$PARENT/teloscope_amd/libteloscan.so" ]; then
        for c in fastq_device_cli bam_device_cli; do
            g++ -std=c++17 -O2 -I "$PARENT/include" "$PARENT/tests/cpp/$c.cpp" -L "$PARENT/teloscope_amd" -lteloscan \
                -Wl,-rpath,"$(cd "$PARENT/teloscope_amd" && pwd)" -pthread -lz -o $TMP/parent_$c || return 1
        done
        echo "parent: $PARENT"
    else
        PARENT=
        echo "NOT RUN: the parent commit's route (no built checkout at ${PARENT:-ab_old/parent})"
    fi
}

: > $WALLS
step() {    # label, configuration, command...: one process under its own time limit; its kept bytes, its wall time, its stage lines
    local label=$1 cfg=$2 t0 t1
    shift 2
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 300 "$@" > $TMP/kept_$cfg 2> $TMP/err_$cfg || { echo "$label $cfg: FAILED"; tail -5 $TMP/err_$cfg; return 1; }
    t1=$(date +%s%N)
    echo "$label $cfg: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
    grep -E "SubsetDevice" $TMP/err_$cfg | sed 's/^/    /'
}
round() {   # label, mode (fastq or bam), input
    local label=$1 mode=$2 in=$3
    if [ -n "$PARENT" ]; then
        if [ $mode = fastq ]; then step "$label" parent $TMP/parent_fastq_device_cli --fastq-subset --device -l 42 --fastq-chunk-bytes $CHUNK $in || return 1
        else step "$label" parent $TMP/parent_bam_device_cli --bam-subset --device -l 42 --bam-chunk-bytes $CHUNK $in || return 1; fi
    fi
    step "$label" one $CLI --$mode-subset --device --devices 0 -l 42 --chunk-bytes $CHUNK $in &&
    step "$label" two $CLI --$mode-subset --device --devices 0,0 -l 42 --chunk-bytes $CHUNK $in &&
    cmp $TMP/kept_one $TMP/kept_two && { [ -z "$PARENT" ] || cmp $TMP/kept_parent $TMP/kept_one; } && echo "$label: kept bytes equal"
}
measure() { # tag, mode, input
    echo "== $1 ($(stat -c %s $3) bytes, chunks of $CHUNK)"
    round "$1 warm-up" $2 $3 && round "$1 run 1" $2 $3 && round "$1 run 2" $2 $3 && round "$1 run 3" $2 $3
}
summary() {
    echo "== minimum / median of the three runs, wall ms"
    python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2)), []).append(int(m.group(3)))
for (enc, cfg), w in sorted(walls.items()):
    print("%-6s %-6s min %6d  median %6d  max %6d" % (enc, cfg, min(w), sorted(w)[len(w) // 2], max(w)))
PY
}
profile() {
    command -v rocprofv3 > /dev/null || { echo "NOT RUN: rocprofv3 (not installed)"; return 0; }
    rm -rf $TMP/read_routes_multi_prof
    timeout -k 10 600 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d $TMP/read_routes_multi_prof -o multi -- \
        $CLI --fastq-subset --device --devices 0,0 -l 42 --chunk-bytes $CHUNK $FQ.bgz > $TMP/kept_prof 2> $TMP/read_routes_multi_prof.log || return 1
    echo "== two contexts on the bgzipped FASTQ under rocprofv3 --kernel-trace --memory-copy-trace --stats"
    echo "kernels:"
    find $TMP/read_routes_multi_prof -name '*kernel_stats.csv' | head -1 | xargs -r head -12 | cut -c1-200
    echo "memory copies (the commit's copy and the carry are the device-to-device ones):"
    find $TMP/read_routes_multi_prof -name '*memory_copy_stats.csv' | head -1 | xargs -r head -8 | cut -c1-200
}

generate && build && measure plain fastq $FQ && measure bgzip fastq $FQ.bgz && measure bam bam $BAM && summary && profile
