"""The device route of the GFA annotation (annotateGfaDevice) against the host route (annotateGfa) of the same binary,
tests/cpp/gfa_device_cli.cpp, on the two seeded graphs of profiles/gfa_annotate_rate.py —

  (a) an assembly cut into segments, one P line per contig (3 Gb and 60 k segments at --scale 1);
  (b) a pathless graph of segments of 50-2 000 bases, a tenth of them telomere-capped (2 M segments at --scale 1)

— each stored as plain text, as BGZF (level 1, 65 280-byte members) and as one gzip stream (level 1).  Per graph and encoding:
a warm-up of each route, then host and device alternating --reps times in one call, both output files compared every time;
minimum / median / maximum of the whole process's wall time and the device route's TS_TIMING stage line of every run.  Then,
in runs of their own, the new kernels' times under `rocprofv3 --kernel-trace --stats` (the device route on graph (b), BGZF, or
its plain text with --trace-plain) and one default bench.py line.
Writes DIR/gfa_device_rate.txt; a stage that was not run is listed as "not measured".

  python profiles/gfa_device_rate.py --out DIR [--work DIR] [--scale 1.0] [--reps 3] [--only a|b] [--no-trace] [--no-bench]
                                     [--trace-only [--trace-plain]]
"""
import argparse
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import gfa_annotate_rate as A  # noqa: E402

KERNELS = ("ts_fastq_count_kernel", "ts_fastq_count_scan_kernel", "ts_fastq_index_kernel", "ts_gfa_tab_count_kernel", "ts_fasta_scan_kernel",
           "ts_gfa_tabs_kernel", "ts_gfa_kinds_kernel", "ts_gfa_frame_scan_kernel", "ts_gfa_tables_kernel", "ts_gfa_gather_kernel",
           "ts_bgzf_inflate", "ts_gather_pieces_kernel", "ts_scan_tiles", "ts_terminal_ends")


def build_cli(work):
    import teloscope_amd  # noqa: F401
    exe = os.path.join(work, "gfa_device_cli")
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gfa_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", exe])
    return exe


def encode(plain, work, tag):
    """-> {encoding: path}: the plain file, BGZF level 1 and one gzip stream level 1."""
    out = {"plain": plain, "bgzip": os.path.join(work, tag + ".bgzf.gfa.gz"), "gzip": os.path.join(work, tag + ".gfa.gz")}
    gz = zlib.compressobj(1, zlib.DEFLATED, 31)
    with open(plain, "rb") as src, open(out["bgzip"], "wb") as b, open(out["gzip"], "wb") as g:
        while True:
            piece = src.read(65280)
            if not piece:
                break
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            payload = co.compress(piece) + co.flush()
            total = 18 + len(payload) + 8
            b.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (total - 1).to_bytes(2, "little") + payload +
                    (zlib.crc32(piece) & 0xFFFFFFFF).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))
            g.write(gz.compress(piece))
        b.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        g.write(gz.flush())
    return out


def run(exe, route, path, outdir):
    shutil.rmtree(outdir, ignore_errors=True)
    os.makedirs(outdir)
    t0 = time.perf_counter()
    r = subprocess.run([exe, route, "-f", path, "-o", outdir], capture_output=True, text=True, timeout=1500,
                       env=dict(os.environ, TS_TIMING="1"))
    wall = (time.perf_counter() - t0) * 1e3
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    stage = [l for l in r.stderr.splitlines() if l.startswith("annotateGfaDevice:")]
    return wall, r.stdout.split(), (stage[0][len("annotateGfaDevice: "):] if stage else "")


def same_outputs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or len(fa) != 2:
        return False
    return all(subprocess.run(["cmp", "-s", os.path.join(a, f), os.path.join(b, f)]).returncode == 0 for f in fa)


def measure(exe, path, work, reps, log):
    host_dir, dev_dir = os.path.join(work, "out_host"), os.path.join(work, "out_device")
    run(exe, "--host", path, host_dir)
    run(exe, "--device", path, dev_dir)
    assert same_outputs(host_dir, dev_dir), "outputs differ (warm-up) on " + path
    host, dev, stages, stats = [], [], [], None
    for _ in range(reps):
        w, f, _ = run(exe, "--host", path, host_dir)
        host.append(w)
        w, g, stage = run(exe, "--device", path, dev_dir)
        dev.append(w)
        stages.append(stage)
        assert f[:5] == g[:5] and same_outputs(host_dir, dev_dir), "outputs differ on " + path
        stats = (f, g)
    log("    host   %8.0f / %8.0f / %8.0f ms   (parse %s, scan %s, write %s ms in run %d)" % (min(host), statistics.median(host), max(host), stats[0][5], stats[0][6], stats[0][7], reps))
    log("    device %8.0f / %8.0f / %8.0f ms   (%s)" % (min(dev), statistics.median(dev), max(dev), stages[0]))
    for k, (w, stage) in enumerate(zip(dev[1:], stages[1:]), 2):
        log("           run %d: %.0f ms   (%s)" % (k, w, stage))
    return stats[0][:5]


def kernel_trace(exe, path, work, log):
    out = os.path.join(work, "rocprof")
    shutil.rmtree(out, ignore_errors=True)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "gfa", "--", exe, "--device", "-f", path, "-o", os.path.join(work, "out_trace")],
                       capture_output=True, text=True, timeout=1500)
    csvs = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not csvs:
        log("  kernel trace: not measured (rocprofv3 exit %d)" % r.returncode)
        return
    import csv
    with open(csvs[0]) as fh:
        rows = list(csv.DictReader(fh))
    log("  kernel (name contains)            calls   total us   mean us")
    for k in KERNELS:
        hit = [r for r in rows if k in r.get("Name", "")]
        if not hit:
            log("  %-32s  not among the recorded rows" % k)
            continue
        calls = sum(int(h["Calls"]) for h in hit)
        total = sum(float(h["TotalDurationNs"]) for h in hit) / 1e3
        log("  %-32s %6d %10.1f %9.1f" % (k, calls, total, total / max(calls, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--work", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--trace-only", action="store_true", help="graph (b) as BGZF under rocprofv3, nothing else")
    ap.add_argument("--trace-plain", action="store_true", help="with --trace-only: graph (b) as plain text")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    work = a.work or tempfile.mkdtemp(prefix="gfa_device_rate_")
    os.makedirs(work, exist_ok=True)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(os.path.join(a.out, "gfa_device_rate.txt"), "w") as fh:     # (kept current: a run that ends early leaves what it measured)
            fh.write("\n".join(lines) + "\n")

    exe = build_cli(work)
    if a.trace_only:
        plain = os.path.join(work, "graph_b.gfa")
        A.write_graph_b(plain, np.random.default_rng(2), a.scale)
        traced = plain if a.trace_plain else encode(plain, work, "graph_b")["bgzip"]
        log("Kernel times of the device route, a run of its own under rocprofv3 --kernel-trace --stats (%s, --scale %g):" % (os.path.basename(traced), a.scale))
        kernel_trace(exe, traced, work, log)
        shutil.rmtree(work, ignore_errors=True)
        return
    log("annotateGfaDevice against annotateGfa of the same binary on one MI355X (profiles/gfa_device_rate.py --scale %g --reps %d)." % (a.scale, a.reps))
    log("Whole-process wall time, minimum / median / maximum of %d alternating runs after a warm-up of each route; both output files compared" % a.reps)
    log("byte for byte after every pair.  Default options.  The device route's stage lines are those of runs 1, 2, ...")
    traced = None
    for which, write, seed in (("a", A.write_graph_a, 1), ("b", A.write_graph_b, 2)):
        if a.only not in (None, which):
            log("graph (%s): not measured" % which)
            continue
        plain = os.path.join(work, "graph_%s.gfa" % which)
        write(plain, np.random.default_rng(seed), a.scale)
        files = encode(plain, work, "graph_" + which)
        head = None
        for enc in ("plain", "bgzip", "gzip"):
            log("graph (%s), %s, %.1f MB on disk:" % (which, enc, os.path.getsize(files[enc]) / 1e6))
            head = measure(exe, files[enc], work, a.reps, log)
        log("  (%s segments, %s ends, %s scanned, %s without sequence, %s nodes; %.1f MB of text)" % (*head, os.path.getsize(plain) / 1e6))
        if which == "b" or a.only == "a":
            traced = files["bgzip"]
        else:
            for f in files.values():
                os.remove(f)
    if a.no_trace or not traced:
        log("kernel times: not measured")
    else:
        log("Kernel times of the device route, a run of its own under rocprofv3 --kernel-trace --stats (%s):" % os.path.basename(traced))
        kernel_trace(exe, traced, work, log)
    if a.no_bench:
        log("default bench line: not measured")
    else:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], capture_output=True, text=True, timeout=900)
        last = [l for l in r.stdout.splitlines() if l.startswith("{")]
        log("default bench line (python bench.py): " + (last[-1] if last else "not measured (exit %d)" % r.returncode))
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
