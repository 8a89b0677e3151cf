"""The device track formatter's arithmetic (teloscope_amd/csrc/track_format_core.h) on the host: compiled by g++ under ASan + UBSan
as a program of its own (tests/cpp/track_format_host.cpp) — the gfx950 kernels of tracks.hip compile the same functions — and
compared, byte for byte, with printf and with the plain-Python reference the GPU tests use (tests/tracktext.py), which is itself
pinned here against harness.format_bed_files on the CPU oracle's windows.  No GPU needed.

Self-check of the program: the core's text equals snprintf("%.6g") for every ratio n / d with 0 <= n <= d <= 2048, n / d for
d in {4096, 65536, 2^22, 2^32 - 1} x n in {1, 2, 3, d / 3, d - 1}, every GC value of windows of up to 2048 bases, k / 1000 for
k <= 2000, -1, 2^20 random floats in [2^-32, 128) and the ends of that range; values outside it are rejected, not printed;
integers 0, 9, 10, 10^k - 1, 10^k, 10^k + 1, 2^32 +- 1, 2^64 - 1 equal snprintf("%llu"); every byte of a text is written once."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import harness as H
from tests import tracktext as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def host_format(tmp_path_factory):
    """-> (the program, the result of its self-check)"""
    d = tmp_path_factory.mktemp("track_core")
    exe = str(d / "track_format_host")
    src = os.path.join(ROOT, "tests", "cpp", "track_format_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe], capture_output=True, timeout=600, env=ENV)
        if r.returncode == 0:
            break
    return exe, r


def test_numbers_equal_printf_under_sanitizers(host_format):
    _, r = host_format
    assert r.returncode == 0 and not r.stderr, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    m = re.fullmatch(rb"ok (\d+) floats (\d+) integers (\d+) rejected\n", r.stdout)
    assert m, r.stdout
    ratios = sum(d + 1 for d in range(1, 2049))
    assert int(m.group(1)) == 2 * ratios + 4 * 5 + 2001 + 10 + (1 << 20) + 3 * 20000
    assert int(m.group(2)) == 3 + 3 * 19 + 3 + 1 and int(m.group(3)) == 12


def host_tracks(exe, tmp_path, records, segs, w, step, r, g, e):
    path = str(tmp_path / "case.bin")
    T.case_file(path, records, segs, w, step, r, g, e)
    p = subprocess.run([exe, "tracks", path], capture_output=True, timeout=300, env=ENV)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode(errors="replace")[-3000:]
    return T.parse_host_output(p.stdout)


def random_case(rng, w, step, lens, abs0=0):
    """segments of the given lengths (0: no windows), names of changing length, records with counts that fit each window"""
    segs, recs, first, at = [], [], 0, abs0
    for i, ln in enumerate(lens):
        n = T.n_windows(ln, step)
        name = (b"seq%d_" % i) + b"x" * (i % 9)
        segs.append((first, n, at, ln, name))
        for k in range(n):
            size = min(w, ln - k * step)
            cuts = np.sort(rng.integers(0, size + 1, size=4))
            a, c, g, t = int(cuts[0]), int(cuts[1] - cuts[0]), int(cuts[2] - cuts[1]), int(cuts[3] - cuts[2])
            fwd, rev = (0, 0) if k % 5 == 0 else (int(rng.integers(0, size + 1)), int(rng.integers(0, size // 2 + 1)))
            can = int(rng.integers(0, fwd + rev + 1))
            recs.append([a, c, g, t, can, fwd + rev - can, fwd, rev])
        first += n
        at += ln + 17
    return np.array(recs, dtype=np.uint32).reshape(-1, 8), segs


@pytest.mark.parametrize("w,step,flags", [(1000, 500, (1, 1, 1)), (7, 3, (1, 1, 1)), (1024, 1024, (0, 1, 1)), (1000, 1000, (1, 0, 0)),
                                          (4194304 * 2, 4194304 * 2, (1, 1, 1))])
def test_core_tracks_equal_the_python_reference(host_format, tmp_path, w, step, flags):
    """The program's second mode: records and a segment table from a file through the core's line functions, against
    tracktext.py — full windows (term table), trailing short windows of every size (host entropy), a window too long for a
    table, empty segments first, in the middle and last, a start that gains a digit inside a segment."""
    exe, _ = host_format
    rng = np.random.default_rng(20261018 + w)
    lens = [0, 3 * w + 17, 1, 0, w - 1, w, w + 1, w + step, 0] + ([w + k for k in range(1, w)] if w == 7 else [5 * w + 3]) + [0]
    records, segs = random_case(rng, w, step, lens, abs0=9_999_000)
    want = T.format_tracks(records, segs, w, step, *flags)
    got = host_tracks(exe, tmp_path, records, segs, w, step, *flags)
    assert got == want
    assert [x is None for x in got] == [not flags[0]] * 3 + [not flags[1], not flags[2]]


@pytest.mark.parametrize("name,flags", [("t2t.fa", "-w 100 -s 50 -r -g -e"), ("gapped_t2t.fa", "-w 64 -s 64 -r -g -e")])
def test_python_reference_equals_the_writer_restatement_on_oracle_windows(name, flags):
    """tracktext.py against harness.format_bed_files (the restatement of writeBEDFile, src/teloscope.cpp:785-812, that
    tests/test_writers.py holds the C++ writer to), on the CPU oracle's windows of two committed FASTAs, one with gaps."""
    from tests.backends import OracleBackend
    fasta = H.golden_path("testFiles/" + name)
    opts = H.parse_cli("%s %s" % (fasta, flags))
    backend = OracleBackend(opts)
    records = H.read_fasta(fasta)
    paths = [H.walk_path(backend, opts, i, h, s) for i, (h, s) in enumerate(records)]
    files = H.format_bed_files(paths, records, opts)
    got = [b""] * T.N_TRACKS
    for pd in paths:
        if pd["windows"] is not None:
            got = [a + b for a, b in zip(got, T.format_windows(pd["header"].encode(), pd["windows"], True, True, True))]
    assert sum(len(pd["windows"]) for pd in paths if pd["windows"] is not None) > 10
    for t, sfx in enumerate(T.SUFFIXES):
        body = files[sfx].split("\n", 1)[1].encode()                 # (without the track line)
        assert got[t] == body, sfx


def test_entry_points_are_declared_and_exported():
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    assert re.search(r"int\s+ts_window_tracks_format\(ts_ctx \*ctx, const uint32_t \*records, uint64_t n, const ts_track_segment \*segs,", hdr)
    assert re.search(r"int\s+ts_scan_segments_tracks\(ts_ctx \*ctx, const ts_segment_in \*segs, size_t n_segs, const char \*const \*names,", hdr)
    assert "void ts_free_track_text(ts_track_text *t);" in hdr and "#define TELOSCAN_ABI_VERSION 4" in hdr
    for sym in ("ts_window_tracks_format", "ts_scan_segments_tracks", "ts_free_track_text"):
        assert sym in K.SYMBOLS and getattr(K.lib(), sym).argtypes is not None
    assert K.lib().ts_abi_version() == 4
    assert K.lib().ts_window_tracks_format(None, None, 0, None, 0, None, 0, None) == K.TS_ERR_INVALID_ARG
    assert K.lib().ts_scan_segments_tracks(None, None, 0, None, None, None, None) == K.TS_ERR_INVALID_ARG
    mirror = open(os.path.join(ROOT, "include", "teloscope_mi355x.hpp")).read()
    assert "scanSegmentsTrackText(" in mirror


def test_kernels_and_host_program_share_one_source():
    kernel = open(os.path.join(CSRC, "tracks.hip")).read()
    assert '#include "track_format_core.h"' in kernel and "tstrack::float_dec(" in kernel and "tstrack::put_prefix(" in kernel
    core = open(os.path.join(CSRC, "track_format_core.h")).read()
    assert not re.search(r"log2f?\(|logf?\(|#include <c?math", kernel + core)      # no device logarithm, no library call
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\btracks\.hip tracks\.cpp\b", mk, re.M) and re.search(r"^HDRS\s*:=.*track_format_core\.h\b", mk, re.M)
    assert "fast-math" not in mk and "-ffp-contract=off" in mk


def test_track_text_cli_builds_and_the_host_float_text_equals_the_stream(tmp_path):
    """tests/cpp/track_text_cli.cpp --check-put: detail::put(float) (the host writer's memoised to_chars) equals operator<<(float)
    for every n / d with d <= 2048, every GC value of sizes <= 2048, k / 1000 for k <= 2000 and -1.  Host only."""
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    exe = T.build_track_cli(tmp_path / "track_text_cli")
    r = subprocess.run([exe, "--check-put"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.fullmatch(r"ok \d+ values\n", r.stdout), r.stdout
