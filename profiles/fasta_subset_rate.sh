#!/bin/bash
# The FASTA read subset, -l 42, through both routes of the C++ mirror (tests/cpp/fasta_subset_cli.cpp: --host = fastaSubset, records
# framed and body lines joined on the host; --device = fastaSubsetDevice, records framed, bases joined into the read batch and
# passing records gathered on the GPU) on the reads of profiles/sam_subset_rate.sh (same generator, same seed), written as FASTA
# two ways: unwrapped (one body line per read) and at width 60.  Each stored as plain text and bgzipped (BGZF members of 65 280
# bytes, zlib level 1).  Per shape and encoding: one warm-up of each route, then the two alternating three times with TS_TIMING=1,
# the kept bytes compared every time; minimum and median of the three whole processes at the end.  Beside it, for context only
# (there is no earlier FASTA read route to compare with): fastqSubsetDevice on the same reads as FASTQ, the same way.  Run on the
# GPU box.
# usage: profiles/fasta_subset_rate.sh [reads] [output file]
set -e
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-100000}
OUT=${2:-profiles/reads/fasta_subset_rate.txt}
TMP=${TMPDIR:-/tmp}
FA=$TMP/reads_fasta_rate
FQ=$TMP/reads_fasta_rate.fq
CLI=$TMP/fasta_subset_cli
FQCLI=$TMP/fastq_device_cli_for_fasta
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
python3 - $N "$FA" "$FQ" <<'PY'
import numpy as np, struct, sys, zlib, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, '.')
from tests import seqgen
n, fa_path, fq_path = int(sys.argv[1]), sys.argv[2], sys.argv[3]
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
def bgzip(text, path):
    def member(a):
        piece = text[a:a + 65280]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        payload = co.compress(piece) + co.flush()
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
                struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    with ThreadPoolExecutor(16) as ex, open(path, 'wb') as fh:               # (zlib releases the interpreter lock)
        for m in ex.map(member, range(0, len(text), 65280), chunksize=64):
            fh.write(m)
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
def fold60(s):                                                                # the read in lines of 60 bases, each with its '\n'
    k, last = divmod(len(s), 60)
    rows = np.empty((k, 61), dtype=np.uint8)
    rows[:, :60] = np.frombuffer(s, dtype=np.uint8, count=k * 60).reshape(k, 60)
    rows[:, 60] = 10
    return rows.tobytes() + (s[k * 60:] + b"\n" if last else b"")
sizes = {}
for shape in ("unwrapped", "w60"):
    parts = []
    for i in range(n):
        s = buf[offs[i]:offs[i + 1]]
        parts += [b'>r%d hifi np=12\n' % i, s + b"\n" if shape == "unwrapped" else fold60(s)]
    text = b"".join(parts)
    del parts
    open("%s.%s.fa" % (fa_path, shape), 'wb').write(text)
    bgzip(text, "%s.%s.fa.bgz" % (fa_path, shape))
    sizes[shape] = len(text)
parts = []
for i in range(n):
    s = buf[offs[i]:offs[i + 1]]
    parts += [b'@r%d\n' % i, s, b'\n+\n', b'I' * len(s), b'\n']
text = b"".join(parts)
del parts
open(fq_path, 'wb').write(text)
bgzip(text, fq_path + '.bgz')
print("reads %d, bases %d, FASTA text %.2f GB unwrapped and %.2f GB at width 60, FASTQ text %.2f GB, each written two ways in %.0f s" % (
    n, int(lens.sum()), sizes["unwrapped"] / 1e9, sizes["w60"] / 1e9, len(text) / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/fasta_subset_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
g++ -std=c++17 -O2 -I include tests/cpp/fastq_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $FQCLI
ls -la $FA.*.fa $FA.*.fa.bgz $FQ $FQ.bgz | awk '{print $5, $9}'
WALLS=$TMP/fasta_subset_walls.txt
: > $WALLS
run() {     # format, route, tag, input: one whole process (the batch planner's lines are left out of the record)
    local t0 t1
    t0=$(date +%s%N)
    if [ $1 = fastq ]; then
        TS_TIMING=1 timeout -k 10 300 $FQCLI --fastq-subset --$2 -l 42 $4 2> $TMP/fasta_rate_stderr.txt > $TMP/kept_$1_$2.txt || { tail -5 $TMP/fasta_rate_stderr.txt; exit 1; }
    else
        TS_TIMING=1 timeout -k 10 300 $CLI --$2 -l 42 $4 2> $TMP/fasta_rate_stderr.txt > $TMP/kept_$1_$2.txt || { tail -5 $TMP/fasta_rate_stderr.txt; exit 1; }
    fi
    t1=$(date +%s%N)
    grep -v '^ts_batch_create:\|^ts_filter_reads:' $TMP/fasta_rate_stderr.txt || true
    echo "$1 $3 $2: wall $(( (t1 - t0) / 1000000 )) ms" | tee -a $WALLS
}
same() {    # the two routes kept the same bytes, or the measurement ends here
    cmp $TMP/kept_fasta_host.txt $TMP/kept_fasta_device.txt || { echo "kept bytes differ"; exit 1; }
    echo "kept bytes equal"
}
for shape in unwrapped w60; do
    for enc in plain bgzip; do
        case $enc in plain) IN=$FA.$shape.fa; FIN=$FQ;; bgzip) IN=$FA.$shape.fa.bgz; FIN=$FQ.bgz;; esac
        echo "== $shape $enc"
        run fasta host "$shape-$enc warm-up" $IN
        run fasta device "$shape-$enc warm-up" $IN
        same
        if [ $shape = unwrapped ]; then run fastq device "$shape-$enc warm-up" $FIN; fi
        for r in 1 2 3; do
            run fasta host "$shape-$enc run $r" $IN
            run fasta device "$shape-$enc run $r" $IN
            same
            if [ $shape = unwrapped ]; then run fastq device "$shape-$enc run $r" $FIN; fi
        done
    done
done
ls -la $TMP/kept_fasta_host.txt $TMP/kept_fasta_device.txt $TMP/kept_fastq_device.txt | awk '{print $5, $9}'
echo "== minimum / median of the three runs, wall ms of the whole process"
python3 - $WALLS <<'PY'
import re, sys
walls = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+) ([\w-]+) run \d (\w+): wall (\d+) ms", line)
    if m:
        walls.setdefault((m.group(2), m.group(1), m.group(3)), []).append(int(m.group(4)))
for (what, fmt, route), w in sorted(walls.items()):
    print("%-16s %-6s %-6s min %6d  median %6d" % (what, fmt, route, min(w), sorted(w)[len(w) // 2]))
PY
rm -f $FA.*.fa $FA.*.fa.bgz $FQ $FQ.bgz
