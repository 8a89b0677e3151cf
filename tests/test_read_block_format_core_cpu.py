"""The read block report's rules (teloscope_amd/csrc/read_block_format_core.h) on the host: tests/cpp/read_block_format_host.cpp,
compiled by g++ under ASan + UBSan with its own main, against plain Python (tests/readblocks.py) — every digit count, names of 0 to
300 bytes, the name rule's edges per front end; the declarations, exports and binding of the new entry points; and the Python
reference itself, pinned and held against the oracle's verdicts on the shared read sets.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import readblocks as B
from tests import readsets as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NEW_SYMBOLS = ("ts_batch_call_read_blocks", "ts_batch_read_blocks", "ts_fastq_chunk_block_lines", "ts_sam_chunk_block_lines",
               "ts_bam_chunk_block_lines", "ts_read_block_lines_format", "ts_read_block_text_stats")


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
    assert "typedef struct ts_read_block" in code
    assert C.sizeof(K.ReadBlock) == 56 and K.ReadBlock.block.offset == 8 and K.READ_BLOCK_DT.itemsize == 56
    # the rule is stated once, names the output as this project's own and the reference columns it mirrors
    assert hdr.count("The read block report") == 1
    at = hdr.index("The read block report")
    rule = hdr[at:hdr.index("*/", at)]
    assert "project's own" in rule and "writeBEDFile" in rule and "src/teloscope.cpp" in rule and "_terminal_telomeres.bed" in rule
    # without a device the calls refuse, they do not crash
    assert lib.ts_batch_call_read_blocks(None, None) == K.TS_ERR_INVALID_ARG
    n = C.c_uint64(0)
    assert lib.ts_batch_read_blocks(None, None, 0, C.byref(n)) == K.TS_ERR_INVALID_ARG
    assert lib.ts_read_block_text_stats(None, None) == K.TS_ERR_INVALID_ARG
    assert lib.ts_read_block_lines_format(None, None, 0, None, None, None, None, 0, None, 0, C.byref(n)) == K.TS_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("read_block_core")
    exe = str(d / "read_block_format_host")
    src = os.path.join(ROOT, "tests", "cpp", "read_block_format_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe], input=b"", capture_output=True, timeout=120, env=ENV)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return exe


def run_cases(exe, cases):
    p = subprocess.run([exe], input="".join(c + "\n" for c in cases).encode(), capture_output=True, timeout=300, env=ENV)
    assert p.returncode == 0 and not p.stderr, (p.stdout + p.stderr).decode(errors="replace")[-3000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == len(cases)
    return out


def hexed(b):
    return b.hex() if b else "-"


def line_cases():
    """(name, (start, block_len, label, fwd, rev, can, noncan), read_len): every digit count of every column, names of 0-300 bytes"""
    cases = []
    u64 = [10 ** d - 1 for d in range(1, 20)] + [10 ** d for d in range(1, 20)] + [0, (1 << 64) - 1, (1 << 63), (1 << 32) - 1, 1 << 32]
    u32 = [10 ** d - 1 for d in range(1, 10)] + [10 ** d for d in range(1, 10)] + [0, (1 << 32) - 1]
    for i, s in enumerate(u64):
        bl = u32[i % len(u32)]
        if s + bl > B.MASK64:
            bl = B.MASK64 - s                                     # end with twenty digits, not wrapped
        cases.append((b"read%d" % i, (s, bl, b"pq"[i & 1:][:1], 1, 2, 3, 4), 5))
    # an end of every digit count from a one-digit start
    for d in range(1, 11):
        cases.append((b"e", (7, min(10 ** d - 8, (1 << 32) - 1) if d > 1 else 1, b"p", 0, 0, 0, 0), 9))
    for col in range(5):                                          # each 32-bit column through every digit count
        for v in u32:
            f = [1, 1, 1, 1, 1]
            f[col] = v
            cases.append((b"n", (12, 34, b"q", f[0], f[1], f[2], f[3]), f[4]))
    for n in list(range(0, 70)) + [127, 128, 129, 255, 256, 257, 299, 300]:
        cases.append((bytes(33 + (j * 7 + n) % 94 for j in range(n)), (n, n + 1, b"p", n, 0, n, 0), 1000 + n))
    cases.append((b"tab\there and space ", (1, 2, b"b", 3, 4, 5, 6), 7))    # (the formatter prints the name's bytes as they are)
    return cases


def test_lines_equal_python_under_sanitizers(host_program):
    cases = line_cases()
    digits = {len(str(c[1][0])) for c in cases} | {len(str((c[1][0] + c[1][1]) & B.MASK64)) for c in cases}
    assert digits >= set(range(1, 21))
    for col in (1, 3, 4, 5, 6):
        assert {len(str(c[1][col])) for c in cases} >= set(range(1, 11)), col
    assert {len(str(c[2])) for c in cases} >= set(range(1, 11))
    assert {len(c[0]) for c in cases} >= set(range(0, 70)) | {300}
    text = ["L %s %d %d %d %d %d %d %d %d" % (hexed(name), row[0], row[1], row[2][0], row[3], row[4], row[5], row[6], read_len)
            for name, row, read_len in cases]
    got = run_cases(host_program, text)
    for (name, row, read_len), g in zip(cases, got):
        exp = B.format_line(name, row, read_len)
        n, h = g.split()
        assert int(n) == len(exp) and bytes.fromhex(h) == exp, (name, row, read_len, g)


def test_name_rules_per_front_end(host_program):
    fastq = [b"@\n", b"@ x\n", b"@a\tb\n", b"@a\r\n", b"@\r\n", b"@name\n", b"@name rest of it\r\n", b"@a\rb\n", b"@a\r \n", b"@" + b"x" * 300 + b" y\n"]
    exp_fastq = [b"", b"", b"a", b"a", b"", b"name", b"name", b"a\rb", b"a\r", b"x" * 300]
    assert [B.fastq_name(h) for h in fastq] == exp_fastq
    sam = [b"\t0\t*\t0", b"q\t0", b"a b\t4", b"x" * 255 + b"\t"]
    exp_sam = [b"", b"q", b"a b", b"x" * 255]
    assert [B.sam_name(s) for s in sam] == exp_sam

    def bam(name):
        rec = bytearray(36)
        rec[12] = len(name) + 1
        return bytes(rec) + name + b"\0" + b"\x88" * 8
    bams = [b"n", b"read/1", b"y" * 254]
    cases = ["F " + hexed(h + b"A") for h in fastq] + ["S " + hexed(s) for s in sam] + ["B " + hexed(bam(n)) for n in bams]
    got = [tuple(int(x) for x in g.split()) for g in run_cases(host_program, cases)]
    assert got[:len(fastq)] == [(1, len(e)) for e in exp_fastq]
    assert got[len(fastq):len(fastq) + len(sam)] == [(0, len(e)) for e in exp_sam]
    assert got[len(fastq) + len(sam):] == [(36, len(n)) for n in bams]
    for h, (off, n), e in zip(fastq, got, exp_fastq):
        assert h[off:off + n] == e


def test_read_blocks_cli_builds_and_refuses_a_route_without_a_device(tmp_path):
    from teloscope_amd import _capi
    libdir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "read_blocks_cli")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "read_blocks_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", exe])
    (tmp_path / "in.fastq").write_bytes(b"@r\n" + b"CCCTAA" * 20 + b"\n+\n" + b"I" * 120 + b"\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for route in ("--host", "--device"):
        p = subprocess.run([exe, "--fastq-subset", route, "--blocks", str(tmp_path / "out.bed"), str(tmp_path / "in.fastq")],
                           stdin=subprocess.DEVNULL, capture_output=True, timeout=120, env=env)
        assert p.returncode == 1 and p.stderr.startswith(b"Error: ") and b"no usable HIP device" in p.stderr, p.stderr
        assert p.stdout == b""
    p = subprocess.run([exe, "in.fastq"], stdin=subprocess.DEVNULL, capture_output=True, timeout=60, env=env)
    assert p.returncode == 1 and b"--fastq-subset, --bam-subset or --sam-subset is required" in p.stderr


def test_ref_report_is_pinned():
    """One read with a forward telomere at its start and a reverse one at its end, by hand: TTAGGG is the reverse unit and CCCTAA the
    forward one of the default set; 50 units are 300 bases, above the read filter's 42."""
    flags = "-l 42"
    oracle = B.read_oracle(flags)
    body = b"ACGTACGTAGCTAGCTAGGATCCGATCGATTCGAGCTA" * 20
    read = b"CCCTAA" * 50 + body + b"TTAGGG" * 50
    text, kept = B.ref_report([(b"both", read), (b"none", body), (b"", b"CCCTAA" * 10)], oracle)
    assert kept == [b"both", b""]
    n = len(read)
    assert text == (b"both\t0\t300\t300\tp\t50\t0\t50\t0\t%d\n" % n + b"both\t%d\t%d\t300\tq\t0\t50\t50\t0\t%d\n" % (n - 300, n, n) +
                    b"\t0\t60\t60\tp\t10\t0\t10\t0\t60\n")


@pytest.mark.parametrize("flags", ["-l 42"] + R.SETS, ids=["tiled"] + R.SET_IDS)
def test_names_in_the_report_are_the_reads_that_pass(flags):
    text, kept = B.set_report(flags)
    reads = R.reads_for(flags)
    passes = R.oracle_passes(flags)
    assert kept == [b"r%d" % i for i, p in enumerate(passes) if p]
    assert 0 < len(kept) < len(reads)
    lines = text.splitlines(keepends=True)
    assert all(ln.endswith(b"\n") and b"\r" not in ln and ln.count(b"\t") == 9 for ln in lines)
    named = []
    for ln in lines:
        f = ln[:-1].split(b"\t")
        assert int(f[2]) == int(f[1]) + int(f[3]) and int(f[2]) <= int(f[9]) and f[4] in (b"p", b"q")
        if not named or named[-1] != f[0]:
            named.append(f[0])
    assert named == kept                                          # a kept record has at least one line, the others none
