"""GFA annotation rate (include/teloscope_mi355x_gfa.hpp through tests/cpp/gfa_cli.cpp) on two seeded synthetic graphs:

  (a) a 3 Gb assembly (tests/seqgen.chromosome contigs) cut into ~60 k segments, one P line per contig;
  (b) a pathless graph of ~2 M segments of 50-2 000 bases, a tenth of them capped with telomeric repeat at one or both ends.

For each graph: the wall time of annotateGfa split into parse, scan and write (one fresh process, so the scan includes the
device's first call).  On (b) also the library call alone, warmed, median of 5: ts_terminal_ends against
ts_scan_segments_blocks (whose terminal blocks the host would then reduce per side; that reduction is timed apart, in numpy).
Kernel times come from a separate run under rocprofv3 (--kernel-only b, --reps 1).

  python profiles/gfa_annotate_rate.py --out DIR [--work DIR] [--only a|b] [--kernel-only b] [--reps 5] [--scale 1.0]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import seqgen  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def build_cli(work):
    import teloscope_amd  # noqa: F401  (builds libteloscan.so)
    exe = os.path.join(work, "gfa_cli")
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gfa_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", exe])
    return exe


def write_graph_a(path, rng, scale):
    total = int(3_000_000_000 * scale)
    n_contigs, per_contig = 24, 2500
    clen = total // n_contigs
    with open(path, "wb") as fh:
        fh.write(b"H\tVN:Z:1.2\n")
        paths = []
        for c in range(n_contigs):
            seq = seqgen.chromosome(rng, clen, telo_repeats=int(rng.integers(100, 2000)), n_its=4)
            cuts = np.unique(rng.integers(1, clen, per_contig - 1))
            bounds = np.concatenate([[0], cuts, [clen]])
            names = []
            for i in range(len(bounds) - 1):
                name = b"c%d_s%d" % (c, i)
                names.append(name + b"+")
                fh.write(b"S\t" + name + b"\t" + seq[bounds[i]:bounds[i + 1]] + b"\n")
            paths.append(b"P\tctg%d\t" % c + b",".join(names) + b"\t*\n")
        fh.writelines(paths)
    return None


def write_graph_b(path, rng, scale):
    n = int(2_000_000 * scale)
    lens = rng.integers(50, 2001, n)
    pool = ACGT[rng.integers(0, 4, size=1 << 26)].tobytes()
    cap = seqgen.mutate(rng, seqgen.repeat_array("CCCTAA", 400), 0.02).tobytes()
    tail = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", 400), 0.02).tobytes()
    offs = rng.integers(0, len(pool) - 2001, n)
    kind = rng.integers(0, 20, n)
    with open(path, "wb") as fh:
        buf = []
        for i in range(n):
            ln = int(lens[i])
            s = pool[offs[i]:offs[i] + ln]
            if kind[i] == 1:
                s = cap[:ln // 2] + s[ln // 2:]
            elif kind[i] == 2:
                s = s[:ln - ln // 3] + tail[:ln // 3]
            buf.append(b"S\tu%d\t%s\n" % (i, s))
            if len(buf) == 65536:
                fh.writelines(buf)
                buf = []
        fh.writelines(buf)
    return n


def run_annotate(exe, gfa, outdir):
    t0 = time.perf_counter()
    r = subprocess.run([exe, "-f", gfa, "-o", outdir], capture_output=True, text=True, timeout=1200)
    wall = (time.perf_counter() - t0) * 1e3
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    f = r.stdout.split()
    return dict(segments=int(f[0]), ends=int(f[1]), scanned=int(f[2]), no_seq=int(f[3]), nodes=int(f[4]),
                parse_ms=float(f[5]), scan_ms=float(f[6]), write_ms=float(f[7]), process_wall_ms=wall)


def read_segments(gfa):
    seqs = []
    with open(gfa, "rb") as fh:
        for line in fh:
            if line.startswith(b"S\t"):
                seqs.append(line.rstrip(b"\n").split(b"\t")[2])
    return seqs


def call_compare(gfa, reps, kernel_only=False):
    """ts_terminal_ends vs ts_scan_segments_blocks on graph (b)'s segments, warmed, median of `reps`"""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import parse_cli, user_input
    seqs = read_segments(gfa)
    n = len(seqs)
    tel = ta.Teloscope(user_input(parse_cli("dummy.gfa")))
    arr = (K.SegmentIn * n)()
    for i, s in enumerate(seqs):
        arr[i].seq = s
        arr[i].len = len(s)
        arr[i].tips_only = 1
    ends = np.zeros((n, 2), dtype=np.uint32)
    pe = ends.ctypes.data_as(C.POINTER(C.c_uint32))
    out = (K.SegmentOut * n)()
    lib = K.lib()

    def t_ends():
        t0 = time.perf_counter()
        assert lib.ts_terminal_ends(tel._ctx.ptr, arr, n, pe) == K.TS_OK
        return (time.perf_counter() - t0) * 1e3

    def t_blocks():
        t0 = time.perf_counter()
        assert lib.ts_scan_segments_blocks(tel._ctx.ptr, arr, n, out, None) == K.TS_OK
        return (time.perf_counter() - t0) * 1e3

    if kernel_only:
        t_ends(); t_blocks(); lib.ts_free_segments(out, n)
        return {}
    t_ends(); t_blocks(); lib.ts_free_segments(out, n)        # warm-up
    te, tb, tr = [], [], []
    for _ in range(reps):
        te.append(t_ends())
        tb.append(t_blocks())
        if tr:
            lib.ts_free_segments(out, n)
            continue
        t0 = time.perf_counter()                             # host reduction of the blocks, per side (once: a Python loop)
        red = np.zeros((n, 2), dtype=np.uint32)
        for i in range(n):
            o = out[i]
            for j in range(o.n_terminal_blocks):
                b = o.terminal_blocks[j]
                side = 0 if b.start <= len(seqs[i]) - (b.start + b.block_len) else 1
                if b.block_len > red[i, side]:
                    red[i, side] = b.block_len
        tr.append((time.perf_counter() - t0) * 1e3)
        lib.ts_free_segments(out, n)
    assert np.array_equal(red, ends), "ts_terminal_ends differs from the reduced blocks"
    return dict(segments=n, ends_with_block=int((ends > 0).any(axis=1).sum()),
                ts_terminal_ends_ms=statistics.median(te), ts_scan_segments_blocks_ms=statistics.median(tb),
                host_reduction_python_ms=tr[0], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--work", default=None)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--kernel-only", choices=["b"], default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    work = a.work or tempfile.mkdtemp(prefix="gfa_rate_")
    os.makedirs(work, exist_ok=True)
    res = {}
    gb = os.path.join(work, "graph_b.gfa")
    if a.kernel_only:
        rng = np.random.default_rng(2)
        write_graph_b(gb, rng, a.scale)
        call_compare(gb, 1, kernel_only=True)
        return
    exe = build_cli(work)
    if a.only in (None, "a"):
        ga = os.path.join(work, "graph_a.gfa")
        t0 = time.perf_counter()
        write_graph_a(ga, np.random.default_rng(1), a.scale)
        res["a"] = dict(bytes=os.path.getsize(ga), generate_s=time.perf_counter() - t0)
        res["a"].update(run_annotate(exe, ga, work))
        os.remove(ga)
    if a.only in (None, "b"):
        t0 = time.perf_counter()
        nseg = write_graph_b(gb, np.random.default_rng(2), a.scale)
        res["b"] = dict(generated_segments=nseg, bytes=os.path.getsize(gb), generate_s=time.perf_counter() - t0)
        res["b"].update(run_annotate(exe, gb, work))
        res["b"]["call_compare"] = call_compare(gb, a.reps)
    with open(os.path.join(a.out, "gfa_annotate_rate.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
