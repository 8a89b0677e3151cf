"""The device match-line formatter's rules (teloscope_amd/csrc/match_format_core.h) on the host: compiled by g++ under ASan + UBSan
as a program of its own (tests/cpp/match_format_host.cpp) — the gfx950 kernels of match_text.hip compile the same functions — and
compared, byte for byte, with snprintf + upper-cased substr and with the plain-Python reference the GPU tests use
(tests/matchtext.py), which is itself pinned here against harness.format_bed_files on the CPU oracle's matches.  No GPU needed."""
import os
import re
import subprocess

import pytest

from tests import harness as H
from tests import matchtext as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NEW_SYMBOLS = ("ts_match_lines_format", "ts_free_match_text", "ts_scan_segments_text", "ts_match_text_stats")


def test_entry_points_are_declared_and_exported():
    """The four new functions and the two new types are in the header, the library exports the functions, the ABI is still 4."""
    import ctypes as C

    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    assert re.search(r"int\s+ts_match_lines_format\(ts_ctx \*ctx, const ts_match \*records, uint64_t n, const ts_match_line_segment \*segs, size_t n_segs,", hdr)
    assert re.search(r"int\s+ts_scan_segments_text\(ts_ctx \*ctx, const ts_segment_in \*segs, size_t n_segs, const char \*const \*names,", hdr)
    assert "void ts_free_match_text(ts_match_text *t);" in hdr and re.search(r"int\s+ts_match_text_stats\(const ts_ctx \*ctx, uint64_t out\[4\]\);", hdr)
    assert re.search(r"#define TS_N_MATCH_FILES 2\b", hdr) and "} ts_match_text;" in hdr and "} ts_match_line_segment;" in hdr
    assert "#define TELOSCAN_ABI_VERSION 4" in hdr
    raw = C.CDLL(K.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in K.SYMBOLS and hasattr(raw, sym) and getattr(K.lib(), sym).argtypes is not None
    assert K.lib().ts_abi_version() == 4 and K.N_MATCH_FILES == 2
    assert C.sizeof(K.MatchText) == 64 and C.sizeof(K.MatchLineSegment) == 56
    assert K.lib().ts_match_lines_format(None, None, 0, None, 0, None, 0, None, 0, None) == K.TS_ERR_INVALID_ARG
    assert K.lib().ts_scan_segments_text(None, None, 0, None, None, None, None, None) == K.TS_ERR_INVALID_ARG
    assert K.lib().ts_match_text_stats(None, None) == K.TS_ERR_INVALID_ARG
    empty = K.MatchText()
    K.lib().ts_free_match_text(C.byref(empty))                      # (a zeroed struct: nothing to free)
    K.lib().ts_free_match_text(None)
    for sym in ("ts_match_lines_format", "ts_scan_segments_text", "ts_match_text_stats"):     # each cites the reference lines it stands in for
        at = hdr.index(sym + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "485-509" in comment and "writeBEDFile" in comment, sym
    assert "src/teloscope.cpp:466-468, 485-509" in hdr
    mirror = open(os.path.join(ROOT, "include", "teloscope_mi355x.hpp")).read()
    assert "scanSegmentsText(" in mirror and "ts_scan_segments_text(" in mirror


@pytest.fixture(scope="module")
def host_format(tmp_path_factory):
    """-> (the program, the result of its self-check)"""
    d = tmp_path_factory.mktemp("match_core")
    exe = str(d / "match_format_host")
    src = os.path.join(ROOT, "tests", "cpp", "match_format_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe], capture_output=True, timeout=600, env=ENV)
        if r.returncode == 0:
            break
    return exe, r


def test_lines_equal_snprintf_under_sanitizers(host_format):
    _, r = host_format
    assert r.returncode == 0 and not r.stderr, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    m = re.fullmatch(rb"ok (\d+) lines (\d+) selections\n", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 12_000 and int(m.group(2)) > 1_000


def host_lines(exe, tmp_path, records, segs, bases, limit):
    path = str(tmp_path / "case.bin")
    M.case_file(path, records, segs, bases, limit)
    p = subprocess.run([exe, "lines", path], capture_output=True, timeout=300, env=ENV)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode(errors="replace")[-3000:]
    return M.parse_host_output(p.stdout)


def test_core_lines_equal_the_python_reference(host_format, tmp_path):
    """The program's second mode: the generated case (tests/matchtext.py: every digit count, every size and name length, the
    edges of the terminal rule, skipped records, a tips-only segment) through the core's functions, against matchtext.py."""
    exe, _ = host_format
    records, segs, bases = M.generated_case()
    want, want_lines = M.format_matches(records, segs, bases, M.CASE_LIMIT)
    got, lines = host_lines(exe, tmp_path, records, segs, bases, M.CASE_LIMIT)
    assert got == want and lines == want_lines
    # what the case is there for
    digits_pos = {len(b"%d" % r[0]) for r in records}
    digits_end = {len(b"%d" % (r[0] + r[1])) for r in records}
    assert digits_pos == set(range(1, 21)) and digits_end == set(range(1, 21))
    assert sum(len(b"%d" % r[0]) != len(b"%d" % (r[0] + r[1])) for r in records) >= 2 * 19
    assert {r[1] for r in records} == set(M.SIZES) and {len(s[5]) for s in segs} == set(M.NAME_LENS)
    assert 0 < lines[1] < sum(1 for r in records if not r[2] & 2) and lines[0] > 100


def test_counted_segments_through_the_core(host_format, tmp_path):
    exe, _ = host_format
    records, segs, bases = M.counted_case([0, 1, 63, 64, 65, 200, 0, 513], long_name=True)
    assert host_lines(exe, tmp_path, records, segs, bases, M.CASE_LIMIT) == M.format_matches(records, segs, bases, M.CASE_LIMIT)


FASTAS = sorted(f for f in os.listdir(os.path.dirname(H.golden_path("testFiles/t2t.fa"))) if f.endswith(".fa"))


# (-m and -m -t 300 with the default patterns, which are all canonical but for one file's; and a set with non-canonical patterns)
@pytest.mark.parametrize("flags", ["-m", "-m -t 300", "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -m -t 300"])
def test_python_reference_equals_the_writer_restatement_on_oracle_matches(flags):
    """matchtext.py against harness.format_bed_files (the restatement of writeBEDFile that tests/test_writers.py holds the C++
    writer to), on the CPU oracle's allMatches of every committed FASTA: the routing into the two files is matchtext.py's own,
    from allMatches and the segment's length."""
    from tests.backends import OracleBackend
    with_matches = with_noncanonical = 0
    for name in FASTAS:
        fasta = H.golden_path("testFiles/" + name)
        opts = H.parse_cli("%s %s" % (fasta, flags))
        backend = OracleBackend(opts)
        records = H.read_fasta(fasta)
        paths = [H.walk_path(backend, opts, i, h, s) for i, (h, s) in enumerate(records)]
        files = H.format_bed_files(paths, records, opts)
        got, n_lines = [b"", b""], [0, 0]
        for pd, (_, seq) in zip(paths, records):
            abs_pos = 0
            for comp in H.path_components(seq):
                if comp[0] != "S":
                    abs_pos += comp[2]
                    continue
                s = comp[2]
                r = backend.scan_segment(s.upper(), abs_pos, False)
                recs = [(int(m["position"]), int(m["match_size"]), M.MATCH_CANONICAL if m["is_canonical"] else 0) for m in r["all_matches"]]
                # (the bases as they lie in the file: matchSeq is upper-cased by the formatter)
                text, lines = M.format_matches(recs, [(0, len(recs), abs_pos, len(s), 0, pd["header"].encode(), False)], s.encode(),
                                               opts.terminal_limit)
                got = [a + b for a, b in zip(got, text)]
                n_lines = [a + b for a, b in zip(n_lines, lines)]
                abs_pos += len(s)
        for f, sfx in enumerate(M.SUFFIXES):
            assert got[f] == files[sfx].encode(), (name, sfx)
        with_matches += n_lines[0] > 0
        with_noncanonical += n_lines[1] > 0
    assert with_matches >= 20 and with_noncanonical >= (2 if "-p" in flags else 1)


def test_kernels_and_host_program_share_one_source():
    kernel = open(os.path.join(CSRC, "match_text.hip")).read()
    assert '#include "match_format_core.h"' in kernel and "tsmatch::select_file(" in kernel and "tsmatch::put_line(" in kernel
    for decode in ("tsmatch::decode_tiled(", "tsmatch::decode_general(", "tsmatch::decode_match("):
        assert decode in kernel
    assert "atomic" not in kernel.split("#include <hip/hip_runtime.h>")[1]      # the text's order is the stream's order
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\bmatch_text\.hip match_text\.cpp\b", mk, re.M) and re.search(r"^HDRS\s*:=.*match_format_core\.h\b", mk, re.M)
