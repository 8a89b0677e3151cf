"""Interleaved paired FASTQ without a device (the rule: include/teloscan.h, "Interleaved paired FASTQ"): the rule's plain-Python
statement (tests/fastqpairs.py: ref_paired_subset) against hand-written expectations for every bullet of the rule; the host
route (detail::fastqSubsetPairedWith) against that statement through tests/cpp/fastq_pairs_host.cpp — a stand-alone program with
a stand-in judge, built by g++ under ASan + UBSan and run directly; the names' core header (fastq_pair_core.h) against Python;
and the declarations, exports and ctypes mirror of the two new entry points."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import fastqchunk as F
from tests import fastqpairs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["ts_fastq_chunk_mates", "ts_fastq_chunk_pair_pass"]
MOTIF = b"TTAGGGTTAGGG"
T = b"TTAGGG" * 6                                    # a read that passes the stand-in judge
N = b"ACGTCA" * 6                                    # one that does not


class MotifFilter:
    """The stand-in judge of tests/cpp/fastq_pairs_host.cpp."""

    def filter(self, reads):
        return [MOTIF in r for r in reads]


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fastq_pairs_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def rec(name, seq, eol=b"\n"):
    return F.record_text(name, seq, eol=eol)


def subset(text):
    out, stats, msg, judged = P.ref_paired_subset(text, MotifFilter())
    return out, stats, msg, [n for n, _ in judged]


# ------------------------------------------------------------------------------------ the statement, bullet by bullet
def test_pairs_are_records_by_parity_and_kept_when_either_mate_passes():
    pairs = [(T, T), (T, N), (N, T), (N, N)]
    text = b"".join(rec(b"p%d/1" % j, a) + rec(b"p%d/2" % j, b) for j, (a, b) in enumerate(pairs))
    out, stats, msg, judged = subset(text)
    assert msg is None and stats == (8, 6)
    assert out == b"".join(rec(b"p%d/1" % j, a) + rec(b"p%d/2" % j, b) for j, (a, b) in enumerate(pairs[:3]))
    # the block report names the written records that passed themselves: a record written only for its mate has no line
    assert judged == [b"p0/1", b"p0/2", b"p1/1", b"p1/2", b"p2/1", b"p2/2"]
    assert [n for n, s in P.ref_paired_subset(text, MotifFilter())[3] if MOTIF in s] == [b"p0/1", b"p0/2", b"p1/1", b"p2/2"]


def test_blank_lines_are_skipped_and_records_are_written_verbatim():
    a, b = rec(b"x 1:N:0", T, eol=b"\r\n"), F.record_text(b"x 2:N:0", N, qual=b"@" + b"+" * 35, plus=b"+x")
    text = a + b"\n\r\n" + b + b"\n\n"
    out, stats, msg, _ = subset(text)
    assert (out, stats, msg) == (a + b, (2, 2), None)


def test_names_end_at_space_tab_cr_and_line_end():
    for end_a, end_b in ((b" 1", b"\t2"), (b"", b" x"), (b"\tq", b"")):
        text = rec(b"read7" + end_a, T) + rec(b"read7" + end_b, N)
        assert subset(text)[2] is None
    text = rec(b"read7", T, eol=b"\r\n") + rec(b"read7/2", N)
    assert subset(text)[2] is None and subset(text)[1] == (2, 2)
    assert subset(rec(b"read7 a", T) + rec(b"read8 a", N))[2] == P.name_error(0)


@pytest.mark.parametrize("case", P.name_cases(), ids=[c[3].replace(" ", "_") for c in P.name_cases()])
def test_mate_names(case):
    a, b, ok, what = case
    assert (P.mate_name(a) == P.mate_name(b)) == ok
    out, stats, msg, _ = subset(rec(a, T) + rec(b, N))
    assert (msg is None) == ok and (msg is None or msg == P.name_error(0)) and (out != b"") == ok, what
    # hand-written, not derived: what the rule's bullets say
    assert P.mate_name(b"a/1") == b"a" and P.mate_name(b"a/2") == b"a" and P.mate_name(b"a/3") == b"a/3"
    assert P.mate_name(b"a/12") == b"a/12" and P.mate_name(b"a/1/") == b"a/1/" and P.mate_name(b"/1") == b"" and P.mate_name(b"a/1/1") == b"a/1"


def test_a_mate_without_bases_is_written_with_its_pair():
    e = rec(b"q/2", b"")
    text = rec(b"q/1", T) + e + rec(b"r/1", N) + rec(b"r/2", b"") + rec(b"s/1", b"") + rec(b"s/2", T) + rec(b"t/1", b"") + rec(b"t/2", b"")
    out, stats, msg, judged = subset(text)
    assert msg is None and stats == (8, 4) and judged == [b"q/1", b"s/2"]
    assert out == rec(b"q/1", T) + e + rec(b"s/1", b"") + rec(b"s/2", T)


def kept(j, first=T, second=N):
    return rec(b"k%d/1" % j, first) + rec(b"k%d/2" % j, second)


def test_errors_the_lowest_offending_place_wins():
    good = kept(0) + kept(1, N, N) + kept(2, N, T)
    written = kept(0) + kept(2, N, T)
    # an odd number of records
    assert subset(good + rec(b"z/1", T))[::2] == (written, P.UNPAIRED)
    # a pair that is not well formed: in the middle, and as the last
    bad = rec(b"m/1", T) + rec(b"n/2", T)
    assert subset(good + bad + kept(3))[::2] == (written, P.name_error(3))
    assert subset(good + bad)[::2] == (written, P.name_error(3))
    # the four record errors at the first and at the second mate: the single valid record in front is never written
    for kind in (F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS):
        broken = F._damage(kind, b"bad")
        assert subset(good + broken + rec(b"bad", T))[::2] == (written, P.record_error(kind, 6))
        assert subset(good + rec(b"bad", T) + broken)[::2] == (written, P.record_error(kind, 7))
    cut = b"@cut\n" + T + b"\n+"                                   # two lines and a half: the input ends inside the record
    assert subset(good + cut)[::2] == (written, P.record_error(F.TRUNCATED, 6))
    assert subset(good + rec(b"cut", T) + cut)[::2] == (written, P.record_error(F.TRUNCATED, 7))
    # a record error wins over the name error of its own pair and of the pairs behind it
    assert subset(good + rec(b"other", T) + F._damage(F.BAD_LENGTHS, b"bad") + bad)[2] == P.record_error(F.BAD_LENGTHS, 7)
    # a name error wholly in front of the record error wins; so it does over the unpaired record
    assert subset(good + bad + kept(4) + F._damage(F.BAD_HEADER, b"bad"))[::2] == (written, P.name_error(3))
    assert subset(good + bad + rec(b"z/1", T))[::2] == (written, P.name_error(3))
    # the refusals of the unpaired route keep their texts
    assert subset(b"")[2] == "FASTQ input is empty" and subset(b"\n" + good)[2] == "FASTQ input must start with '@'"


# ------------------------------------------------------------------------------------ the host route and the core header
def host_cases():
    """name -> complete text: the rule's corners, LF and CRLF, and the error inputs, each with a kept pair in front."""
    cases = {}
    for eol_name, eol in (("lf", b"\n"), ("crlf", b"\r\n")):
        k = lambda j, a=T, b=N: rec(b"k%d/1" % j, a, eol) + rec(b"k%d/2" % j, b, eol)     # noqa: E731
        good = k(0) + k(1, N, N) + k(2, N, T) + k(3, T, T)
        bad = rec(b"m/1", T, eol) + rec(b"n/2", T, eol)
        many = b"".join(rec(b"g%d 1:N:0" % j, (T if j % 3 == 0 else N) + b"ACGT" * (j % 50), eol) + rec(b"g%d 2:N:0" % j, (T if j % 5 == 0 else N) * (1 + j % 7), eol)
                        for j in range(120))
        c = {
            "every kind of pair": good, "many pairs": many, "one pair": k(0), "one pair, neither passes": k(0, N, N),
            "blank lines": k(0) + eol + b"\n" + k(1, N, T) + b"\n\n", "no final newline": (good + k(4))[:-len(eol)],
            "mates without bases": rec(b"q/1", T, eol) + rec(b"q/2", b"", eol) + rec(b"r/1", b"", eol) + rec(b"r/2", b"", eol) + rec(b"s/1", b"", eol) + rec(b"s/2", T, eol),
            "names of every case": b"".join(rec(a, T, eol) + rec(b, N, eol) for a, b, ok, _ in P.name_cases() if ok),
            "odd record count": good + rec(b"z/1", T, eol), "odd record count behind many": many + rec(b"z/1", T, eol),
            "mismatch in the middle": good + bad + k(5), "mismatch last": good + bad, "mismatch first": bad + good,
            "mismatch behind many": many + bad + many,
            "record error behind a mismatch": good + bad + k(5) + F._damage(F.BAD_HEADER, b"bad"),
            "mismatch behind a record error": good + rec(b"o", T, eol) + F._damage(F.BAD_LENGTHS, b"bad") + bad,
            "truncated first mate": good + b"@cut" + eol + T + eol + b"+", "truncated second mate": good + rec(b"cut", T, eol) + b"@cut" + eol + T,
            "only a header": b"@lonely",
        }
        for kind in (F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS):
            c["%s at the first mate" % F.MESSAGES[kind]] = many + F._damage(kind, b"bad") + rec(b"bad", T, eol) + k(7)
            c["%s at the second mate" % F.MESSAGES[kind]] = many + rec(b"bad", T, eol) + F._damage(kind, b"bad") + k(7)
        cases.update({"%s, %s" % (name, eol_name): text for name, text in c.items()})
    cases["empty"] = b""
    cases["a blank line first"] = b"\n" + rec(b"a", T) + rec(b"a", T)
    return cases


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fastq_pairs_host") / "fastq_pairs_host"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-pthread", os.path.join(ROOT, "tests", "cpp", "fastq_pairs_host.cpp"), "-o", str(exe), "-lz"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return str(exe)


@pytest.mark.parametrize("name", sorted(host_cases()))
def test_host_route_under_asan_and_ubsan(host, tmp_path, name):
    """Every case, mapped and gzipped through the block reader, blocks of 64 bytes to the whole file, one record to a thousand per
    batch: one answer, the statement's; the sanitizers have nothing to say."""
    text = host_cases()[name]
    p = tmp_path / "case.fq"
    p.write_bytes(text)
    r = subprocess.run([host, "subset", str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-600:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    out, stats, msg, _ = P.ref_paired_subset(text, MotifFilter())
    assert lines[0] == ("error " + msg if msg else "ok %d %d" % stats), (lines, msg, stats)
    assert open(str(p) + ".out", "rb").read() == out
    assert lines[1].startswith("runs ") and int(lines[1].split()[1]) > 50


def test_host_cases_hold_what_they_name():
    cases = host_cases()
    messages = {name: P.ref_paired_subset(text, MotifFilter())[2] for name, text in cases.items()}
    for eol in ("lf", "crlf"):
        assert messages["odd record count, " + eol] == P.UNPAIRED and messages["odd record count behind many, " + eol] == P.UNPAIRED
        assert messages["mismatch in the middle, " + eol] == messages["mismatch last, " + eol] == messages["record error behind a mismatch, " + eol] == P.name_error(4)
        assert messages["mismatch first, " + eol] == P.name_error(0)
        assert messages["mismatch behind a record error, " + eol] == P.record_error(F.BAD_LENGTHS, 9)
        assert messages["truncated first mate, " + eol] == P.record_error(F.TRUNCATED, 8)
        assert messages["truncated second mate, " + eol] == P.record_error(F.TRUNCATED, 9)
        for kind in (F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS):
            assert messages["%s at the first mate, %s" % (F.MESSAGES[kind], eol)] == P.record_error(kind, 240)
            assert messages["%s at the second mate, %s" % (F.MESSAGES[kind], eol)] == P.record_error(kind, 241)
        for name, text in cases.items():
            if name.endswith(", " + eol) and messages[name] and "only a header" not in name and "mismatch first" not in name:
                assert P.ref_paired_subset(text, MotifFilter())[0], name            # a kept pair stands in front of every error
        assert b"\r" not in cases["many pairs, lf"] and cases["many pairs, crlf"].count(b"\r\n") == 4 * 240
        assert messages["many pairs, " + eol] is None


def test_core_header_equality_against_python(host, tmp_path):
    """tspair::mates over the name cases, written as records behind one another at every alignment, LF and CRLF and with
    comments behind the names: the core header the kernel compiles answers what Python answers."""
    cases = P.name_cases()
    for eol, end in ((b"\n", b""), (b"\r\n", b""), (b"\n", b" 1:N:0"), (b"\n", b"\tx y")):
        text = b"".join(rec(a + end, T[:20 + i % 7], eol) + rec(b + end, N, eol) for i, (a, b, _, _) in enumerate(cases))
        p = tmp_path / "names.fq"
        p.write_bytes(text)
        r = subprocess.run([host, "names", str(p)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stdout[-600:] + r.stderr[-2000:]
        assert [l == "1" for l in r.stdout.splitlines()] == [ok for _, _, ok, _ in cases]


def test_header_declares_and_library_exports_the_entry_points():
    """Fails without the feature: include/teloscan.h states the rule and declares the entry points, libteloscan.so exports them
    and the binding names them."""
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "Interleaved paired FASTQ" in hdr and P.UNPAIRED in flat and "do not have the same name" in flat
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        assert getattr(K.lib(), name).argtypes, name                 # the ctypes mirror loads them with their signatures
    assert lib.ts_abi_version() == 4
    host = open(os.path.join(ROOT, "include", "teloscope_mi355x_reads_host.hpp")).read()
    device = open(os.path.join(ROOT, "include", "teloscope_mi355x_io.hpp")).read()
    assert "fastqSubsetPaired" in host and "fastqSubsetPairedDevice" in device and "FastqPairChunkSteps" in device
