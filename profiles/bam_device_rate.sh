#!/bin/bash
# --bam-subset -l 42 through both routes of the C++ mirror (tests/cpp/bam_device_cli.cpp: --host = bamSubset, zlib on the host
# threads; --device = bamSubsetDevice, BGZF members inflated on the GPU) on the BAM of profiles/bam_subset_rate.sh (same
# generator, same seed): one warm-up of each, then the two alternating three times with TS_TIMING=1, the kept bytes compared
# every time; then the device route once more under rocprofv3 --kernel-trace --stats (a run of its own, no counters) for the
# kernels' own times.  Run on the GPU box.   usage: profiles/bam_device_rate.sh [reads] [output file]
set -e
cd "$(dirname "$0")/.."
N=${1:-120000}
OUT=${2:-profiles/bam/bam_device_rate.txt}
TMP=${TMPDIR:-/tmp}
BAM=$TMP/reads_device_rate.bam
CLI=$TMP/bam_device_cli
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
python3 - $N "$BAM" <<'PY'
import numpy as np, struct, sys, zlib, time
sys.path.insert(0, '.')
from tests import seqgen
n = int(sys.argv[1])
rng = np.random.default_rng(43)
lens = np.clip(rng.normal(15000, 3000, size=n), 1000, 40000).astype(np.int64)
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
with open(sys.argv[2], 'wb') as fh:
    pend = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0))
    def flush(final=False):
        global pend
        while len(pend) >= 65280 or (final and pend):
            piece = bytes(pend[:65280]); del pend[:65280]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            payload = co.compress(piece) + co.flush()
            fh.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
                     struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    for i in range(n):
        s = nib[offs[i]:offs[i + 1]]
        L = len(s)
        if L & 1:
            s = np.concatenate((s, np.zeros(1, dtype=np.uint8)))
        packed = ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes()
        name = b"m64011_%d/ccs" % i
        qual = rng.integers(20, 60, size=L, dtype=np.uint8).tobytes()       # noisy qualities: compress like real ones (badly)
        tags = b"npC\x08rqf" + struct.pack("<f", 0.999)
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 255, 4680, 0, 4, L, -1, -1, 0) + name + b"\0" + packed + qual + tags
        pend += struct.pack("<i", len(body)) + body
        raw_bytes += 4 + len(body)
        flush()
    flush(True)
    fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
print("reads %d, bases %d, uncompressed BAM %.2f GB, written in %.0f s" % (n, int(lens.sum()), raw_bytes / 1e9, time.time() - t0))
PY
g++ -std=c++17 -O2 -I include tests/cpp/bam_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
run() {     # route, tag
    local t0 t1
    t0=$(date +%s%N); TS_TIMING=1 timeout -k 10 300 $CLI --bam-subset --$1 -l 42 $BAM > $TMP/kept_$1.bam; t1=$(date +%s%N)
    echo "$2 $1: wall $(( (t1 - t0) / 1000000 )) ms"
}
run host warm-up
run device warm-up
cmp $TMP/kept_host.bam $TMP/kept_device.bam && echo "kept bytes equal"
for r in 1 2 3; do
    run host "run $r"
    run device "run $r"
    cmp $TMP/kept_host.bam $TMP/kept_device.bam && echo "kept bytes equal"
done
ls -la $BAM $TMP/kept_host.bam $TMP/kept_device.bam | awk '{print $5, $9}'
if command -v rocprofv3 > /dev/null; then
    rm -rf $TMP/bam_device_prof
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/bam_device_prof -o bam_device -- $CLI --bam-subset --device -l 42 $BAM > $TMP/kept_prof.bam 2> $TMP/bam_device_prof.log
    echo "kernel stats (rocprofv3 --kernel-trace --stats):"
    find $TMP/bam_device_prof -name '*kernel_stats.csv' | head -1 | xargs -r head -12 | cut -c1-200
fi
