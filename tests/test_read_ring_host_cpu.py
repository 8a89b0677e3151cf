"""The dealing, carry, ordering and error layer of the read routes on several contexts (include/teloscope_mi355x_ring.hpp)
against stand-in contexts made of host buffers: tests/cpp/read_ring_host.cpp, a stand-alone program, built with ASan + UBSan and a
second time with TSan (where the toolchain has that runtime) and run once each.  It compares 1-4 contexts, every chunk size of a
40-record text, a record that is not valid at every position and a writer that fails at every write with the loop on one
context; the sanitizers must have nothing to say."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "read_ring_host.cpp")


def build(out, sanitize):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=" + sanitize,
                           "-fno-sanitize-recover=all", "-pthread", SOURCE, "-o", str(out)], capture_output=True, text=True)


def run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-600:] + r.stderr[-2000:]
    lines = r.stdout.split()
    assert r.stdout.splitlines()[-1] == "ok" and {"every-cut", "errors", "failing-writer"} <= set(lines), r.stdout


def test_ring_on_host_buffers_under_asan_and_ubsan(tmp_path):
    b = build(tmp_path / "read_ring_host", "address,undefined")
    assert b.returncode == 0, b.stderr[-2000:]
    run(tmp_path / "read_ring_host")


def test_ring_on_host_buffers_under_tsan(tmp_path):
    b = build(tmp_path / "read_ring_host_tsan", "thread")
    if b.returncode != 0 and ("tsan" in b.stderr or "-fsanitize=thread" in b.stderr):
        pytest.skip("this toolchain has no ThreadSanitizer runtime")
    assert b.returncode == 0, b.stderr[-2000:]
    run(tmp_path / "read_ring_host_tsan")
