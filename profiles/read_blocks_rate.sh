#!/bin/bash
# The read block report's cost, through tests/cpp/read_blocks_cli.cpp: --fastq-subset -l 42 on the reads of
# profiles/fastq_device_rate.sh (same generator, same seed: 100 000 HiFi-like reads, a telomere in 0.5 % of them) and on the same
# reads with a telomere at the start of EVERY read (a telomere-enriched library: every read passes, the whole input is echoed and
# every read has lines).  Per data set: one warm-up, then host and device route, each without and with --blocks, alternating three
# times with TS_TIMING=1; the subset's bytes compared between the four every time and the two reports with each other; minimum and
# median of the three whole processes at the end.
# Then every device route WITHOUT the report against binaries built from the parent commit (the same reads as FASTQ, SAM and BAM):
# PARENT_BIN names a directory that holds the parent's libteloscan.so and its fastq_device_cli, sam_device_cli and bam_device_cli,
# linked against that library (git worktree add <dir> <parent>; make -C <dir>/teloscope_amd/csrc; g++ ... as below).  Without
# PARENT_BIN that part is left out.  Run on the GPU box.
# usage: [PARENT_BIN=dir] profiles/read_blocks_rate.sh [reads] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-100000}
OUT=${2:-profiles/reads/read_blocks_rate.txt}
TMP=${TMPDIR:-/tmp}
D=$TMP/read_blocks_rate
CLI=$D/read_blocks_cli
mkdir -p "$(dirname "$OUT")" $D
exec > >(tee "$OUT") 2>&1
python3 - $N $D "${PARENT_BIN:+with_parent}" <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
n, d, parent = int(sys.argv[1]), sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == "with_parent"
rng = np.random.default_rng(43)
lens = np.clip(rng.normal(15000, 3000, size=n), 1000, 40000).astype(np.int64)
pool = seqgen.random_dna(rng, int(lens.sum()))
offs = np.concatenate(([0], np.cumsum(lens)))
def plant(which):
    for i in which:
        ln = int(rng.integers(300, 8000))
        t = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", ln // 6 + 1), 0.01)[:min(ln, lens[i])]
        pool[offs[i]:offs[i] + len(t)] = t
def fastq(path):
    buf = pool.tobytes()
    parts = []
    for i in range(n):
        s = buf[offs[i]:offs[i + 1]]
        parts += [b'@m64011_%d/ccs np=12\n' % i, s, b'\n+\n', b'I' * len(s), b'\n']
    text = b"".join(parts)
    open(path, 'wb').write(text)
    return len(text)
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
t0 = time.time()
plant(np.flatnonzero(rng.random(n) < 0.005))
size = fastq(d + "/default.fq")
print("default.fq written, %.0f s" % (time.time() - t0), flush=True)
if parent:
    buf = pool.tobytes()
    parts = [b"@HD\tVN:1.6\tSO:unsorted\n"]
    for i in range(n):
        s = buf[offs[i]:offs[i + 1]]
        parts += [b'm64011_%d/ccs\t4\t*\t0\t0\t*\t*\t0\t0\t' % i, s, b'\t', b'I' * len(s), b'\tnp:i:12\n']
    open(d + "/default.sam", 'wb').write(b"".join(parts))
    print("default.sam written, %.0f s" % (time.time() - t0), flush=True)
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
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes() + b"\x28" * L
        parts += [struct.pack("<i", len(body)), body]
    bgzip(b"".join(parts), d + "/default.bam")
    print("default.bam written, %.0f s" % (time.time() - t0), flush=True)
    del parts, nib
plant(range(n))
fastq(d + "/every.fq")
print("reads %d, bases %d, FASTQ text %.2f GB; written in %.0f s" % (n, int(lens.sum()), size / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/read_blocks_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
WALLS=$D/walls.txt
: > $WALLS
run() {     # binary, mode, route, tag (label of the record), input, output name, further options: one whole process
    local t0 t1 bin=$1 mode=$2 route=$3 tag=$4 in=$5 name=$6
    shift 6
    t0=$(date +%s%N)
    TS_TIMING=1 timeout -k 10 300 $bin --$mode-subset --$route -l 42 "$@" $in 2> $D/stderr.txt > $D/kept_$name || { tail -5 $D/stderr.txt; exit 1; }
    t1=$(date +%s%N)
    grep -v '^ts_batch_create:\|^ts_filter_reads:' $D/stderr.txt || true
    echo "$tag: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
for set in default every; do
    IN=$D/$set.fq
    echo "== FASTQ, $set: a telomere in $([ $set = default ] && echo '0.5 % of the reads' || echo 'every read')"
    run $CLI fastq device "$set warm-up device" $IN warm
    for r in 1 2 3; do
        run $CLI fastq host "$set run $r host plain" $IN host_plain
        run $CLI fastq host "$set run $r host report" $IN host_report --blocks $D/host.bed
        run $CLI fastq device "$set run $r device plain" $IN device_plain
        run $CLI fastq device "$set run $r device report" $IN device_report --blocks $D/device.bed --stats
        cmp $D/kept_host_plain $D/kept_device_plain && cmp $D/kept_host_plain $D/kept_host_report && cmp $D/kept_host_plain $D/kept_device_report
        cmp $D/host.bed $D/device.bed
        echo "subset bytes equal four ways, reports equal: $(wc -l < $D/device.bed) lines, $(wc -c < $D/device.bed) bytes"
    done
done
if [ -n "$PARENT_BIN" ]; then
    echo "== device routes without the report: this tree (read_blocks_cli) against the parent commit's binaries, default reads"
    for fmt in fastq sam bam; do
        case $fmt in fastq) IN=$D/default.fq;; sam) IN=$D/default.sam;; bam) IN=$D/default.bam;; esac
        run $PARENT_BIN/${fmt}_device_cli $fmt device "$fmt warm-up parent" $IN parent
        run $CLI $fmt device "$fmt warm-up this" $IN this
        for r in 1 2 3; do
            run $PARENT_BIN/${fmt}_device_cli $fmt device "$fmt run $r parent" $IN parent
            run $CLI $fmt device "$fmt run $r this" $IN this
            cmp $D/kept_parent $D/kept_this && echo "subset bytes equal"
        done
    done
fi
echo "== minimum / median of the three runs, wall ms of the whole process"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) run \d (.+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(1), m.group(2)), []).append(int(m.group(3)))
for (a, b), w in walls.items():
    print("%-8s %-14s min %6d  median %6d   (%s)" % (a, b, min(w), sorted(w)[len(w) // 2], " ".join(map(str, w))))
PY
rm -rf $D
