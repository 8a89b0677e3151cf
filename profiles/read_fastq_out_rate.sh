#!/bin/bash
# FASTQ out of the BAM and SAM subsets, through tests/cpp/read_fastq_out_cli.cpp: -l 42 on the 100 000 HiFi-like reads of the
# other read records (profiles/read_blocks_rate.sh's generator and seed) written as BAM and as SAM, every second read with FLAG 16;
# once with a telomere in 0.5 % of the reads (the default fraction) and once with one at the start of EVERY read (every read passes
# and the whole input leaves as FASTQ).  Per format and data set: one warm-up, then device FASTQ-out, device native (the verbatim
# subset) and host FASTQ-out, alternating three times with TS_TIMING=1; the FASTQ text compared between host and device every
# time; minimum and median of the three whole processes at the end.  Then the new kernels' time from a rocprofv3 --kernel-trace
# --stats run of its own (every read passing, BAM and SAM).
# Then the unchanged native device routes against binaries built from the parent commit, on the default sets: PARENT_BIN names a
# directory that holds the parent's libteloscan.so and its read_blocks_cli, linked against that library (git worktree add <dir>
# <parent>; make -C <dir>/teloscope_amd/csrc; g++ ... as below), the two alternating, who goes first alternating too.  Without
# PARENT_BIN that part is left out; with AB_ONLY=1 it is the only part that runs.  Run on the GPU box.
# usage: [PARENT_BIN=dir] [AB_ONLY=1] profiles/read_fastq_out_rate.sh [reads] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-100000}
OUT=${2:-profiles/reads/read_fastq_out_rate.txt}
TMP=${TMPDIR:-/tmp}
D=$TMP/read_fastq_out_rate
CLI=$D/read_fastq_out_cli
mkdir -p "$(dirname "$OUT")" $D
exec > >(tee "$OUT") 2>&1
python3 - $N $D ${AB_ONLY:+ab_only} <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
n, d = int(sys.argv[1]), sys.argv[2]
rng = np.random.default_rng(43)
lens = np.clip(rng.normal(15000, 3000, size=n), 1000, 40000).astype(np.int64)
pool = seqgen.random_dna(rng, int(lens.sum()))
offs = np.concatenate(([0], np.cumsum(lens)))
def plant(which):
    for i in which:
        ln = int(rng.integers(300, 8000))
        t = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", ln // 6 + 1), 0.01)[:min(ln, lens[i])]
        pool[offs[i]:offs[i] + len(t)] = t
def bgzip(data, path):
    def member(a):
        piece = data[a:a + 65280]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        payload = co.compress(piece) + co.flush()
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
                struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    with ThreadPoolExecutor(16) as ex, open(path, 'wb') as fh:               # (zlib releases the interpreter lock)
        for m in ex.map(member, range(0, len(data), 65280), chunksize=64):
            fh.write(m)
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
def sam(path):
    buf = pool.tobytes()
    parts = [b"@HD\tVN:1.6\tSO:unsorted\n"]
    for i in range(n):
        s = buf[offs[i]:offs[i + 1]]
        parts += [b'm64011_%d/ccs\t%d\t*\t0\t0\t*\t*\t0\t0\t' % (i, 16 if i & 1 else 4), s, b'\t', b'I' * len(s), b'\tnp:i:12\n']
    open(path, 'wb').write(b"".join(parts))
def bam(path):
    code = np.zeros(256, dtype=np.uint8)
    for ch, v in zip(b"=ACMGRSVTWYHKDBN", range(16)):
        code[ch] = v
    nib = code[pool]
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    parts = [b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)]
    for i in range(n):
        s = nib[offs[i]:offs[i + 1]]
        L = len(s)
        if L & 1:
            s = np.concatenate((s, np.zeros(1, dtype=np.uint8)))
        name = b"m64011_%d/ccs" % i
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 16 if i & 1 else 4, L, -1, -1, 0) + name + b"\0" + \
            ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes() + b"\x28" * L
        parts += [struct.pack("<i", len(body)), body]
    bgzip(b"".join(parts), path)
t0 = time.time()
plant(np.flatnonzero(rng.random(n) < 0.005))
sam(d + "/default.sam"); bam(d + "/default.bam")
print("default.sam and default.bam written, %.0f s" % (time.time() - t0), flush=True)
if len(sys.argv) > 3:                        # (the comparison with the parent alone: the default sets)
    sys.exit(0)
plant(range(n))
sam(d + "/every.sam"); bam(d + "/every.bam")
print("reads %d, bases %d; written in %.0f s" % (n, int(lens.sum()), time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/read_fastq_out_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
WALLS=$D/walls.txt
: > $WALLS
run() {     # tag (label of the record), output name, the command: one whole process
    local t0 t1 tag=$1 name=$2
    shift 2
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 300 "$@" 2> $D/stderr.txt > $D/kept_$name || { tail -5 $D/stderr.txt; exit 1; }
    t1=$(date +%s%N)
    grep -v '^ts_batch_create:\|^ts_filter_reads:' $D/stderr.txt || true
    echo "$tag: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
for fmt in $([ -n "$AB_ONLY" ] || echo bam sam); do
    for set in default every; do
        IN=$D/$set.$fmt
        echo "== $fmt, $set: a telomere in $([ $set = default ] && echo '0.5 % of the reads' || echo 'every read'); input $(wc -c < $IN) bytes"
        run "$fmt $set warm-up device" warm $CLI --$fmt --device -l 42 $IN
        for r in 1 2 3; do
            run "$fmt $set run $r device fastq-out" device_fastq $CLI --$fmt --device --stats -l 42 $IN
            run "$fmt $set run $r device native" device_native $CLI --$fmt --device --native -l 42 $IN
            run "$fmt $set run $r host fastq-out" host_fastq $CLI --$fmt --host -l 42 $IN
            cmp $D/kept_host_fastq $D/kept_device_fastq
            echo "FASTQ text equal, host and device: $(wc -c < $D/kept_device_fastq) bytes, $(( $(wc -l < $D/kept_device_fastq) / 4 )) records; native subset $(wc -c < $D/kept_device_native) bytes"
        done
    done
done
echo "== the new kernels, every read passing: rocprofv3 --kernel-trace --stats, a run of its own per format"
for fmt in $([ -n "$AB_ONLY" ] || echo bam sam); do
    rm -rf $D/trace
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace -o t -- $CLI --$fmt --device -l 42 $D/every.$fmt > /dev/null 2> $D/stderr.txt || { tail -5 $D/stderr.txt; exit 1; }
    echo "-- $fmt"
    find $D/trace -name '*kernel_stats.csv' | head -1 | xargs -r head -1
    find $D/trace -name '*kernel_stats.csv' | head -1 | xargs -r grep 'ts_read_fastq' | cut -c1-260
done
if [ -n "$PARENT_BIN" ]; then
    echo "== the unchanged native device routes: this tree (read_fastq_out_cli --native) against the parent commit's read_blocks_cli, default reads"
    for fmt in bam sam; do
        IN=$D/default.$fmt
        parent() { run "$fmt native $1 parent" parent $PARENT_BIN/read_blocks_cli --$fmt-subset --device -l 42 $IN; }
        this() { run "$fmt native $1 this" this $CLI --$fmt --device --native -l 42 $IN; }
        parent warm-up; this warm-up
        for r in 1 2 3; do                      # (who goes first alternates from round to round)
            if [ $r = 2 ]; then this "run $r"; parent "run $r"; else parent "run $r"; this "run $r"; fi
            cmp $D/kept_parent $D/kept_this && echo "subset bytes equal"
        done
    done
fi
echo "== minimum / median of the three runs, wall ms of the whole process"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+ \w+) run \d (.+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2)), []).append(int(m.group(3)))
for (a, b), w in walls.items():
    print("%-12s %-18s min %6d  median %6d  max %6d   (%s)" % (a, b, min(w), sorted(w)[len(w) // 2], max(w), " ".join(map(str, w))))
native = {k: v for k, v in walls.items() if k[0].endswith("native")}
for fmt in ("bam", "sam"):
    p, t = native.get((fmt + " native", "parent")), native.get((fmt + " native", "this"))
    if p and t:
        m = sorted(t)[1]
        where = "inside" if min(p) <= m <= max(p) else "BELOW (faster than)" if m < min(p) else "ABOVE (slower than)"
        print("%s native device route: this tree's median %d ms lies %s the parent's own spread %d .. %d ms" % (fmt, m, where, min(p), max(p)))
PY
rm -rf $D
