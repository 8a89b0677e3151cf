#!/bin/bash
# The output side of --bam-subset on the device route (tests/cpp/bam_deflate_cli.cpp): --deflate host (zlib level 6 on the host
# threads inside the writer's turn, the default) against --deflate device (ts_bam_chunk_gather_bgzf: the passing records
# deflated and framed on the GPU), on a generated HiFi-like BAM (the generator of profiles/bam_device_rate.sh, smaller) at the
# default telomeric fraction and with every read telomeric (TELOMERIC=1: the output is as large as the input).
#   1. compression ratio: the device encoder's payload bytes on the BAM's own 0xff00 cuts (ts_bgzf_deflate) against Python's zlib
#      at level 1 and level 6 on the same cuts;
#   2. time: host and device alternating three times on one context and on --devices 0,0, whole process (wall) plus the TS_TIMING
#      stage lines; the unchanged bam_device_cli --device of this tree beside them, and where PARENT_CLI names a bam_device_cli
#      built from the parent commit (with its own libteloscan.so) that one too: the default path must not have moved;
#   3. the device form once more under rocprofv3 --kernel-trace --stats, for the deflate kernels' own time.
# Run on the GPU box.   usage: [TELOMERIC=f] [PARENT_CLI=path] profiles/bgzf_deflate_rate.sh [reads] [output file]
set -e
cd "$(dirname "$0")/.."
N=${1:-12000}
OUT=${2:-profiles/bam/bgzf_deflate_rate.txt}
TMP=${TMPDIR:-/tmp}
CLI=$TMP/bam_deflate_cli
OLD=$TMP/bam_device_cli
mkdir -p "$(dirname "$OUT")"
exec > >(tee "$OUT") 2>&1
g++ -std=c++17 -O2 -I include tests/cpp/bam_deflate_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $CLI
g++ -std=c++17 -O2 -I include tests/cpp/bam_device_cli.cpp -L teloscope_amd -lteloscan -Wl,-rpath,$PWD/teloscope_amd -pthread -lz -o $OLD
generate() {    # telomeric fraction, file
python3 - $N "$2" "$1" <<'PY'
import numpy as np, struct, sys, zlib, time
sys.path.insert(0, '.')
from tests import seqgen
n, frac = int(sys.argv[1]), float(sys.argv[3])
rng = np.random.default_rng(43)
lens = np.clip(rng.normal(15000, 3000, size=n), 1000, 40000).astype(np.int64)
pool = seqgen.random_dna(rng, int(lens.sum()))
offs = np.concatenate(([0], np.cumsum(lens)))
for i in np.flatnonzero(rng.random(n) < frac):
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
print("telomeric fraction %g: reads %d, bases %d, uncompressed BAM %.2f GB, written in %.0f s" % (frac, n, int(lens.sum()), raw_bytes / 1e9, time.time() - t0))
PY
}
ratio() {       # file
timeout -k 10 300 python3 - "$1" <<'PY'
import struct, sys, zlib
sys.path.insert(0, '.')
import teloscope_amd as ta
from teloscope_amd.bgzf import deflate_blocks
from teloscope_amd.cli import parse_cli, user_input
data = open(sys.argv[1], 'rb').read()
plain, pos = [], 0
while pos < len(data):
    total = struct.unpack_from("<H", data, pos + 16)[0] + 1
    plain.append(zlib.decompress(data[pos + 18:pos + total - 8], -15))
    pos += total
plain = b"".join(plain)[:256 << 20]
cuts = [plain[i:i + 0xff00] for i in range(0, len(plain), 0xff00)]
def z(level):
    t = 0
    for c in cuts:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        t += len(co.compress(c) + co.flush())
    return t
tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=0))
members = deflate_blocks(tel._ctx.ptr, plain, 0xff00)
device = len(members) - 26 * len(cuts)
l1, l6 = z(1), z(6)
print("compression ratio on %d cuts of 0xff00 (%d plain bytes): payload bytes device %d, zlib level 1 %d, zlib level 6 %d; device / level 1 = %.4f, device / level 6 = %.4f"
      % (len(cuts), len(plain), device, l1, l6, device / l1, device / l6))
PY
}
run() {     # binary, tag, args...
    local bin=$1 tag=$2 t0 t1
    shift 2
    t0=$(date +%s%N); TS_TIMING=1 timeout -k 10 300 $bin --bam-subset "$@" -l 42 $BAM > $TMP/kept_$tag.bam; t1=$(date +%s%N)
    echo "$tag: wall $(( (t1 - t0) / 1000000 )) ms, $(stat -c %s $TMP/kept_$tag.bam) bytes written"
}
for FRACTION in ${TELOMERIC:-0.005} 1; do
    BAM=$TMP/reads_deflate_rate_$FRACTION.bam
    generate $FRACTION $BAM
    ratio $BAM
    run $CLI host --deflate host          # warm-up of each
    run $CLI device --deflate device
    for r in 1 2 3; do
        echo "--- telomeric $FRACTION, run $r, one context"
        run $OLD default --device
        if [ -n "$PARENT_CLI" ]; then run $PARENT_CLI parent --device; cmp $TMP/kept_parent.bam $TMP/kept_host.bam && echo "parent's bytes equal --deflate host's"; fi
        run $CLI host --deflate host
        run $CLI device --deflate device
        cmp $TMP/kept_default.bam $TMP/kept_host.bam && echo "default bytes equal --deflate host's"
        echo "--- telomeric $FRACTION, run $r, --devices 0,0"
        run $CLI host2 --deflate host --devices 0,0
        run $CLI device2 --deflate device --devices 0,0
        cmp $TMP/kept_device.bam $TMP/kept_device2.bam && echo "device bytes equal on one and two contexts"
    done
    if command -v rocprofv3 > /dev/null; then       # the kernels' own times: a run of its own, no counters
        rm -rf $TMP/bgzf_deflate_prof
        timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TMP/bgzf_deflate_prof -o bgzf_deflate -- $CLI --bam-subset --deflate device -l 42 $BAM > $TMP/kept_prof.bam 2> $TMP/bgzf_deflate_prof.log
        echo "kernel stats, telomeric $FRACTION, --deflate device (rocprofv3 --kernel-trace --stats):"
        find $TMP/bgzf_deflate_prof -name '*kernel_stats.csv' | head -1 | xargs -r head -12 | cut -c1-200
    fi
    python3 -c "
import gzip, sys
a, b = (gzip.open(p).read() for p in sys.argv[1:3])
print('inflated outputs equal' if a == b else 'INFLATED OUTPUTS DIFFER', len(a), len(b))" $TMP/kept_host.bam $TMP/kept_device.bam
done
