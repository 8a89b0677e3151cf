"""FASTQ out of the BAM and SAM subsets (teloscope_amd/csrc/read_fastq_format_core.h) on the host: literal known answers held
against the plain-Python rule (tests/readfastq.py) and against tests/cpp/read_fastq_format_host.cpp, compiled by g++ under
ASan + UBSan with its own main; that program against Python on generated records; the declarations, exports and binding of the new
entry points; and the round trip FASTQ -> BAM / SAM -> FASTQ through the host routes against fastqSubset on the original (that
case needs a device behind the filter and is marked gpu)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from tests import readfastq as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NEW_SYMBOLS = ("ts_bam_chunk_gather_fastq", "ts_sam_chunk_gather_fastq", "ts_read_fastq_text_stats")


def test_new_entry_points_are_declared_exported_and_bound():
    """Fails without the feature: none of the names exists before it."""
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(K.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert sym in K.SYMBOLS and hasattr(lib, sym), sym
    assert lib.ts_abi_version() == 4 and "#define TELOSCAN_ABI_VERSION 4" in hdr
    assert re.search(r"#define\s+TS_FASTQ_OUT_RESTORE_STRAND\s+1u", code)
    # the rule is stated once, above the entry points, as this project's own
    assert hdr.count("FASTQ out of the BAM and SAM subsets") == 1
    at = hdr.index("FASTQ out of the BAM and SAM subsets")
    rule = hdr[at:hdr.index("*/", at)]
    assert "project's own" in rule and "primaries" in rule and "stored-SEQ coordinates" in rule and "No BAM header" in rule
    assert at < hdr.index("int ts_bam_chunk_gather_fastq")
    # without a chunk or a context the calls refuse, they do not crash
    n = C.c_uint64(0)
    assert lib.ts_bam_chunk_gather_fastq(None, None, 0, None, 0, None, 0, C.byref(n), C.byref(n), None) == K.TS_ERR_INVALID_ARG
    assert lib.ts_sam_chunk_gather_fastq(None, None, 0, None, 0, None, 0, C.byref(n), C.byref(n), None) == K.TS_ERR_INVALID_ARG
    assert lib.ts_read_fastq_text_stats(None, None) == K.TS_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("read_fastq_core")
    exe = str(d / "read_fastq_format_host")
    src = os.path.join(ROOT, "tests", "cpp", "read_fastq_format_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe, "--constants"], capture_output=True, timeout=120, env=ENV)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return exe, d


def run_cases(host_program, cases):
    """cases: [(kind, flags, record bytes)] -> the texts"""
    exe, d = host_program
    path = d / "cases"
    path.write_text("".join("%s %d %s\n" % (k, f, b.hex() if b else "-") for k, f, b in cases))
    p = subprocess.run([exe, str(path)], capture_output=True, timeout=300, env=ENV)
    assert p.returncode == 0 and not p.stderr, (p.stdout + p.stderr).decode(errors="replace")[-3000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == len(cases)
    texts = []
    for row in out:
        n, h = row.split()
        texts.append(bytes.fromhex(h))
        assert int(n) == len(texts[-1])
    return texts


def python_text(kind, flags, rec):
    return Q.bam_text(rec, flags) if kind == "B" else Q.sam_text(rec, flags)


def known_answers():
    """(kind, flags, record, the text, written out)"""
    R = Q.RESTORE_STRAND
    bam, sam = Q.bam_record, Q.sam_line
    all16 = list(range(16))
    return [
        # all 16 codes, forward and reversed; reversed without the flag bit, and with it when the caller wants the stored form
        ("B", R, bam(b"r", 0, all16, all16), b"@r\n=ACMGRSVTWYHKDBN\n+\n!\"#$%&'()*+,-./0\n"),
        ("B", R, bam(b"r", 16, all16, all16), b"@r\nNVHMDRWABSYCKGT=\n+\n0/.-,+*)('&%$#\"!\n"),
        ("B", 0, bam(b"r", 16, all16, all16), b"@r\n=ACMGRSVTWYHKDBN\n+\n!\"#$%&'()*+,-./0\n"),
        ("B", R, bam(b"r", 0x900 | 16, all16, all16), b"@r\nNVHMDRWABSYCKGT=\n+\n0/.-,+*)('&%$#\"!\n"),
        # an odd and an even L reversed
        ("B", R, bam(b"odd", 16, [1, 2, 4], [0, 1, 2]), b"@odd\nCGT\n+\n#\"!\n"),
        ("B", R, bam(b"even", 16, [1, 1, 2, 4], [5, 6, 7, 8]), b"@even\nCGTT\n+\n)('&\n"),
        ("B", R, bam(b"one", 16, [2], [40]), b"@one\nG\n+\nI\n"),
        # QUAL 0xFF; QUAL bytes 92, 93, 94 and 254
        ("B", R, bam(b"", 4, [1, 2, 4], None), b"@\nACG\n+\n!!!\n"),
        ("B", R, bam(b"", 16, [1, 2, 4], None), b"@\nCGT\n+\n!!!\n"),
        ("B", R, bam(b"sat", 4, [8, 8, 8, 8], [92, 93, 94, 254]), b"@sat\nTTTT\n+\n}~~~\n"),
        ("B", R, bam(b"cig", 4, [1, 15], [1, 2], n_cigar=2, tail=b"NMC\x00"), b"@cig\nAN\n+\n\"#\n"),
        # SAM QUAL "*" at L = 1 and at L = 5, with and without tags behind it
        ("S", R, sam(b"q", b"4", b"A", b"*"), b"@q\nA\n+\n!\n"),
        ("S", R, sam(b"q", b"4", b"A", b"*", tags=b"NM:i:0"), b"@q\nA\n+\n!\n"),
        ("S", R, sam(b"q", b"4", b"ACGTN", b"*"), b"@q\nACGTN\n+\n!!!!!\n"),
        ("S", R, sam(b"q", b"16", b"ACGTN", b"*", tags=b"XX:Z:*"), b"@q\nNACGT\n+\n!!!!!\n"),
        ("S", R, sam(b"q", b"4", b"A", b"+"), b"@q\nA\n+\n+\n"),
        # SAM FLAG 16, 0016, x, empty and 1040
        ("S", R, sam(b"f", b"16", b"AAC", b"123"), b"@f\nGTT\n+\n321\n"),
        ("S", R, sam(b"f", b"0016", b"AAC", b"123"), b"@f\nGTT\n+\n321\n"),
        ("S", R, sam(b"f", b"x", b"AAC", b"123"), b"@f\nAAC\n+\n123\n"),
        ("S", R, sam(b"f", b"", b"AAC", b"123"), b"@f\nAAC\n+\n123\n"),
        ("S", R, sam(b"f", b"1040", b"AAC", b"123"), b"@f\nGTT\n+\n321\n"),
        ("S", 0, sam(b"f", b"16", b"AAC", b"123"), b"@f\nAAC\n+\n123\n"),
        ("S", R, sam(b"f", b"16x", b"AAC", b"123"), b"@f\nGTT\n+\n321\n"),
        ("S", R, sam(b"f", b"0000000016", b"AAC", b"123"), b"@f\nAAC\n+\n123\n"),       # nine digits are read: 1
        # lower case and U in SAM SEQ; bytes that are no letter
        ("S", R, sam(b"", b"16", b"acgUuN.=xT", b"0123456789"), b"@\nAx=.NaAcgt\n+\n9876543210\n"),
        ("S", R, sam(b"", b"0", b"acgUuN.=xT", b"0123456789"), b"@\nacgUuN.=xT\n+\n0123456789\n"),
        ("S", R, sam(b"i", b"16", b"MRVHKYBDSWmrvhkybdsw", b"I" * 20), b"@i\nwshvrmdbykWSHVRMDBYK\n+\n" + b"I" * 20 + b"\n"),
        # CRLF lines: the '\r' is no part of QUAL, of "*" or of a tag
        ("S", R, sam(b"c", b"16", b"AC", b"12", eol=b"\r\n"), b"@c\nGT\n+\n21\n"),
        ("S", R, sam(b"c", b"4", b"AC", b"*", eol=b"\r\n"), b"@c\nAC\n+\n!!\n"),
        ("S", R, sam(b"c", b"4", b"A", b"*", eol=b"\r\n"), b"@c\nA\n+\n!\n"),
        ("S", R, sam(b"c", b"4", b"AC", b"12", tags=b"", eol=b"\r\n"), b"@c\nAC\n+\n12\n"),      # the line ends at a tab
        ("S", R, sam(b"c", b"4", b"AC", b"12", tags=b""), b"@c\nAC\n+\n12\n"),
    ]


def strip_nl(kind, rec):
    return rec[:-1] if kind == "S" and rec.endswith(b"\n") else rec


def test_known_answers_in_python():
    for kind, flags, rec, exp in known_answers():
        assert python_text(kind, flags, rec) == exp, (kind, flags, rec)


def test_known_answers_under_sanitizers(host_program):
    cases = known_answers()
    got = run_cases(host_program, [(k, f, strip_nl(k, r)) for k, f, r, _ in cases])
    for (kind, flags, rec, exp), g in zip(cases, got):
        assert g == exp, (kind, flags, rec)


def generated_cases():
    rng = random.Random(11)
    cases = []
    lengths = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000]
    for i, n in enumerate(lengths * 2):
        name = bytes(rng.randrange(33, 127) for _ in range([0, 1, 7, 16, 254][i % 5]))
        flag = rng.choice([0, 4, 16, 20, 0x910, 0x900, 0xffff])
        codes = [rng.randrange(16) for _ in range(n)]
        qual = None if i % 6 == 5 else [rng.choice([0, 1, 40, 92, 93, 94, 127, 128, 254, 255 if j else 0]) for j in range(n)]
        for flags in (0, Q.RESTORE_STRAND):
            cases.append(("B", flags, Q.bam_record(name, flag, codes, qual, n_cigar=i % 3, tail=b"\xff" * (i % 4))))
        seq = bytes(rng.choice(b"ACGTNacgtnUuMRWSYKVHDB=.*-x") for _ in range(n))
        if seq == b"*":
            seq = b"A"
        sq = b"*" if i % 6 == 5 else bytes(rng.randrange(33, 127) for _ in range(n))
        if n == 1 and sq == b"*":
            sq = b"*"                                              # (missing, by the rule)
        field = rng.choice([b"0", b"4", b"16", b"20", b"2320", b"016", b"", b"-16", b"16.5", b"65535", b"123456789012"])
        tags = [None, b"", b"NM:i:1\tXX:Z:a\tb"][i % 3]
        for flags in (0, Q.RESTORE_STRAND):
            cases.append(("S", flags, Q.sam_line(name.replace(b"\t", b"_"), field, seq, sq, tags=tags, eol=b"\r" if i % 4 == 1 else b"")))
    return cases


def test_host_program_equals_python_on_generated_records(host_program):
    cases = generated_cases()
    assert len(cases) > 100
    got = run_cases(host_program, cases)
    reversed_seen = 0
    for (kind, flags, rec), g in zip(cases, got):
        exp = python_text(kind, flags, rec)
        assert g == exp, (kind, flags, rec)
        reversed_seen += python_text(kind, 0, rec) != exp
    assert reversed_seen > 20


def test_the_piece_size_is_a_named_constant(host_program):
    exe, _ = host_program
    out = subprocess.run([exe, "--constants"], capture_output=True, timeout=60, env=ENV).stdout.decode().split()
    assert out[0] == "piece_bytes" and int(out[1]) >= 64 and int(out[1]) % 16 == 0
    core = open(os.path.join(ROOT, "teloscope_amd", "csrc", "read_fastq_format_core.h")).read()
    assert re.search(r"constexpr uint32_t kPieceBytes = %su;" % out[1], core)


def build_cli(name, out_dir):
    from teloscope_amd import _capi
    libdir = os.path.dirname(_capi.LIB_PATH)
    exe = str(out_dir / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def fastq_out_cli(tmp_path_factory):
    return build_cli("read_fastq_out_cli", tmp_path_factory.mktemp("read_fastq_out_cli"))


def test_read_fastq_out_cli_builds_and_refuses_a_route_without_a_device(fastq_out_cli, tmp_path):
    exe = fastq_out_cli
    (tmp_path / "in.sam").write_bytes(Q.sam_line(b"r", b"16", b"CCCTAA" * 20, b"I" * 120))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for route in ("--host", "--device"):
        p = subprocess.run([exe, "--sam", route, str(tmp_path / "in.sam")], stdin=subprocess.DEVNULL, capture_output=True, timeout=120, env=env)
        assert p.returncode == 1 and p.stderr.startswith(b"Error: ") and b"no usable HIP device" in p.stderr, p.stderr
        assert p.stdout == b""
    p = subprocess.run([exe, "in.sam"], stdin=subprocess.DEVNULL, capture_output=True, timeout=60, env=env)
    assert p.returncode == 1 and b"--bam or --sam is required" in p.stderr


@pytest.mark.gpu
def test_round_trip_through_the_host_routes_equals_fastq_subset(fastq_out_cli, tmp_path):
    """A FASTQ whose names hold no space, written as BAM and as SAM by the tests' builder, forward and with FLAG 16 and SEQ and
    QUAL stored reversed: bamSubsetFastq and samSubsetFastq give the bytes fastqSubset gives on the original, under the same
    options.  The expectation comes from the FASTQ front end, not from this feature's code."""
    from tests import readblocks as B
    from tests import readsets as S
    flags = "-l 42"
    rng = random.Random(5)
    reads = [r for r in S.reads_for(flags) if r]
    records = [(b"read/%d:x" % i, r, bytes(rng.randrange(33, 127) for _ in r)) for i, r in enumerate(reads)]
    fastq = b"".join(Q.text_of(n, b, q) for n, b, q in records)
    (tmp_path / "in.fastq").write_bytes(fastq)
    native = build_cli("read_blocks_cli", tmp_path)
    cli = fastq_out_cli
    common = ["--host", "--reads-per-batch", "37", "--chunk-bytes", "65536"] + flags.split()
    p = subprocess.run([native, "--fastq-subset", str(tmp_path / "in.fastq")] + common, stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    exp = p.stdout
    assert 0 < exp.count(b"\n") // 4 < len(records) and exp.count(b"\n") % 4 == 0
    for reverse in (False, True):
        (tmp_path / "in.bam").write_bytes(B.bgzf(Q.bam_header() + Q.fastq_as_bam_records(records, reverse), 3000))
        (tmp_path / "in.sam").write_bytes(Q.fastq_as_sam(records, reverse))
        for kind in ("bam", "sam"):
            p = subprocess.run([cli, "--" + kind, str(tmp_path / ("in." + kind))] + common, stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
            assert p.returncode == 0, p.stderr
            assert p.stdout == exp, (kind, reverse)
