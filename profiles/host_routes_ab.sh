#!/bin/bash
# The host read routes (fastqSubset, bamSubset, samSubset: include/teloscope_mi355x_reads_host.hpp) of this tree against those of
# the parent commit, whole processes: tests/cpp/manifest_cli.cpp (--fastq-subset, --bam-subset) and tests/cpp/sam_device_cli.cpp
# (--sam-subset --host), each built twice — from PARENT (a checkout of the parent commit; its libteloscan.so is built there if it
# is missing) and from this tree, each against its own library; a program that is already there under BIN is not built again.  The
# inputs are those of profiles/chunk_steps_ab.sh (same generator, same seed), a fifth of its reads by default: the FASTQ as plain
# text (above 64 MiB: mapped, its records found by splitFastqRecords) and as gzip (bgzipped: members zlib reads one after the
# other, the block path), the BAM, and the SAM of the same reads.  Per route and input: one warm-up of parent and child, then ROUNDS
# rounds of parent, child, parent again ("parent2": the parent against itself, measured the same way), the kept bytes compared with
# the parent's warm-up every time.  At the end the medians, the parent's own range over both of its series, and whether the child's
# median lies inside it; then bench.py once (it runs none of these routes).  Run on the GPU box.
# (The record in profiles/reads/host_routes_ab.txt has fastq-gzip 103 ms below the parent's median, 32 ms below its range.  The parent's two FASTQ blocks
# were std::vector<char>, zero-filled when resized to 513 MiB each; BlockReader's are new char[].  Filling and then writing two such
# vectors against two such arrays costs about 0.4 s more on one host thread, part of it behind the reader thread in the route;
# that this is the whole of the 103 ms is supposed, not measured in the route.)
# usage: profiles/host_routes_ab.sh PARENT [reads] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
PARENT=${1:?usage: profiles/host_routes_ab.sh PARENT [reads] [output file]}
PARENT=$(cd "$PARENT" && pwd)
N=${2:-20000}
OUT=${3:-profiles/reads/host_routes_ab.txt}
ROUNDS=${ROUNDS:-7}
TMP=${TMPDIR:-/tmp}/host_routes_ab
BIN=${BIN:-$TMP}
FQ=$TMP/reads.fq
SAM=$TMP/reads.sam
BAM=$TMP/reads.bam
mkdir -p "$(dirname "$OUT")" $TMP $BIN/parent $BIN/child
exec > >(tee "$OUT") 2>&1
BUILDS=
[ -f $PARENT/teloscope_amd/libteloscan.so ] || make -s -C $PARENT/teloscope_amd/csrc -j16
[ -f teloscope_amd/libteloscan.so ] || make -s -C teloscope_amd/csrc -j16
for tree in parent child; do
    case $tree in parent) SRC=$PARENT;; child) SRC=$PWD;; esac
    for cli in manifest_cli sam_device_cli; do
        [ -x $BIN/$tree/$cli ] && continue
        g++ -std=c++17 -O2 -I $SRC/include $SRC/tests/cpp/$cli.cpp -L $SRC/teloscope_amd -lteloscan -Wl,-rpath,$SRC/teloscope_amd -pthread -lz -o $BIN/$tree/$cli &
        BUILDS="$BUILDS $!"
    done
done
[ -z "$BUILDS" ] || wait $BUILDS        # (not a bare wait: that would wait for the tee above as well)
for tree in parent child; do for cli in manifest_cli sam_device_cli; do [ -x $BIN/$tree/$cli ]; done; done
python3 - $N "$FQ" "$SAM" "$BAM" <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
n, fq_path, sam_path, bam_path = int(sys.argv[1]), sys.argv[2], sys.argv[3], sys.argv[4]
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
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
def member(piece):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    payload = co.compress(piece) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
            struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
def bgzip(text, path):
    with ThreadPoolExecutor(16) as ex, open(path, 'wb') as fh:               # (zlib releases the interpreter lock)
        for m in ex.map(lambda a: member(text[a:a + 65280]), range(0, len(text), 65280), chunksize=64):
            fh.write(m)
        fh.write(EOF_MARKER)
parts = []
for i in range(n):
    s = buf[offs[i]:offs[i + 1]]
    parts += [b'@r%d\n' % i, s, b'\n+\n', b'I' * len(s), b'\n']
text = b"".join(parts)
open(fq_path, 'wb').write(text)
bgzip(text, fq_path + '.gz')
parts = [b"@HD\tVN:1.6\tSO:unsorted\n@PG\tID:gen\tPN:sam_subset_rate\n"]
for i in range(n):
    s = buf[offs[i]:offs[i + 1]]
    parts += [b'r%d\t4\t*\t0\t0\t*\t*\t0\t0\t' % i, s, b'\t', b'I' * len(s), b'\tRG:Z:hifi\tnp:i:12\n']
text = b"".join(parts)
del parts
open(sam_path, 'wb').write(text)
del text
code = np.zeros(256, dtype=np.uint8)
for ch, v in zip(b"=ACMGRSVTWYHKDBN", range(16)):
    code[ch] = v
nib = code[pool]
header = b"@HD\tVN:1.6\tSO:unknown\n"
plain = [b"BAM\1" + struct.pack("<i", len(header)) + header + struct.pack("<i", 0)]
for i in range(n):
    s = nib[offs[i]:offs[i + 1]]
    L = len(s)
    if L & 1:
        s = np.concatenate((s, np.zeros(1, dtype=np.uint8)))
    packed = ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes()
    name = b"m64011_%d/ccs" % i
    qual = rng.integers(20, 60, size=L, dtype=np.uint8).tobytes()           # noisy qualities: compress like real ones (badly)
    tags = b"npC\x08rqf" + struct.pack("<f", 0.999)
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + packed + qual + tags
    plain += [struct.pack("<i", len(body)), body]
bgzip(b"".join(plain), bam_path)
print("reads %d, bases %d: FASTQ as text and gzip, the SAM and the BAM, written in %.0f s" % (n, int(lens.sum()), time.time() - t0))
PY
ls -la $FQ $FQ.gz $SAM $BAM | awk '{print $5, $9}'
WALLS=$TMP/walls.txt
: > $WALLS
run() {     # configuration, who (parent|child|parent2), tag, the command behind the tree's directory: one whole process
    local conf=$1 who=$2 tag=$3 tree=${2%2} t0 t1
    shift 3
    t0=$(date +%s%N)
    timeout -k 10 300 $BIN/$tree/"$@" > $TMP/kept_$who.out 2> $TMP/stderr_$who.txt || { echo "$conf $who $tag: failed"; tail -5 $TMP/stderr_$who.txt; return 1; }
    t1=$(date +%s%N)
    echo "$conf $who $tag: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # who kept the bytes the parent's warm-up kept, or the measurement ends here
    cmp $TMP/kept_warm.out $TMP/kept_$1.out || { echo "kept bytes differ ($1)"; return 1; }
}
ab() {      # configuration, then the command
    local conf=$1 r
    shift
    echo "== $conf"
    run $conf parent warm-up "$@" && cp $TMP/kept_parent.out $TMP/kept_warm.out && run $conf child warm-up "$@" && same child || exit 1
    for r in $(seq $ROUNDS); do
        run $conf parent "run $r" "$@" && same parent && run $conf child "run $r" "$@" && same child && run $conf parent2 "run $r" "$@" && same parent2 || exit 1
    done
    echo "kept bytes equal every time ($(stat -c %s $TMP/kept_warm.out) bytes)"
}
ab fastq-plain manifest_cli --fastq-subset -l 42 $FQ
ab fastq-gzip manifest_cli --fastq-subset -l 42 $FQ.gz
ab bam manifest_cli --bam-subset -l 42 $BAM
ab sam sam_device_cli --sam-subset --host -l 42 $SAM
echo "== wall ms of the $ROUNDS runs: the parent's range over its two series and its median, the child's median, child - parent"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\S+) (\w+) run \d+: wall (\d+) ms", line)
    if m:
        walls.setdefault(m.group(1), {}).setdefault(m.group(2), []).append(int(m.group(3)))
median = lambda w: sorted(w)[len(w) // 2]
for conf, w in walls.items():
    both = w["parent"] + w["parent2"]
    a, c = median(both), median(w["child"])
    print("%-12s parent %5d .. %5d  median %5d  child %5d  child - parent %+5d  %s" % (conf, min(both), max(both), a, c, c - a,
          "within the parent's range" if min(both) <= c <= max(both) else "below the parent's range" if c < min(both) else "ABOVE the parent's range"))
PY
rm -f $FQ $FQ.gz $SAM $BAM
echo "== bench.py (the assembly scan: none of the routes above)"
timeout -k 10 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 2> /dev/null | tail -1
