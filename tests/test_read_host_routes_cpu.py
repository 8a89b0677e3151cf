"""The host routes of the read subsets (include/teloscope_mi355x_reads_host.hpp: fastqSubset, samSubset / samSubsetFastq, bamSubset /
bamSubsetFastq and the block reader under them) without a device: tests/cpp/read_host_routes_host.cpp, a stand-alone program that
links zlib and pthread only, built with ASan + UBSan and a second time with TSan (where the toolchain has that runtime) and run once
each.  Its judge keeps a read exactly when its bases contain TTAGGGTTAGGG; what is expected comes from a whole-text statement of
each format written in the program.  It runs the block reader at every block size and with a fill that throws at every call, FASTQ
as a plain file and as gzip over block sizes and batch sizes, texts cut at every byte of the last record and one per failure, SAM
over every block size with plain and FASTQ out and a bad line of each kind, and a 3 MB BAM whose 1.2 MB record exceeds the
headroom; the sanitizers must have nothing to say."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "read_host_routes_host.cpp")
CASES = {"block-reader-every-size", "block-reader-failing-fill", "fastq-every-block", "fastq-failures", "fastq-first-byte",
         "sam-every-block", "sam-failures", "bam-large-record", "bam-ends"}


def build(out, sanitize):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=" + sanitize,
                           "-fno-sanitize-recover=all", "-pthread", SOURCE, "-o", str(out), "-lz"], capture_output=True, text=True)


def run(exe, work):
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-600:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == "ok" and CASES <= set(r.stdout.split()), r.stdout


def test_host_routes_under_asan_and_ubsan(tmp_path):
    b = build(tmp_path / "read_host_routes_host", "address,undefined")
    assert b.returncode == 0, b.stderr[-2000:]
    run(tmp_path / "read_host_routes_host", tmp_path / "files")


def test_host_routes_under_tsan(tmp_path):
    b = build(tmp_path / "read_host_routes_host_tsan", "thread")
    if b.returncode != 0 and ("tsan" in b.stderr or "-fsanitize=thread" in b.stderr):
        pytest.skip("this toolchain has no ThreadSanitizer runtime")
    assert b.returncode == 0, b.stderr[-2000:]
    run(tmp_path / "read_host_routes_host_tsan", tmp_path / "files")
