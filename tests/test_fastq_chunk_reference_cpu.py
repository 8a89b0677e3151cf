"""Without a device: the plain-Python FASTQ walk of tests/fastqchunk.py (what tests/test_gpu_fastq_chunk.py holds the device
walk against) pinned on every committed FASTQ input and on the generators' edge and error cases; the C-ABI of the device
route declared and exported; tests/cpp/fastq_device_cli.cpp builds and refuses to run without a device."""
import ctypes as C
import glob
import gzip
import os
import re
import shlex
import subprocess

import pytest

from tests import fastqchunk as F
from tests import harness as H
from tests.backends import OracleReadFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = sorted(glob.glob(os.path.join(H.GOLDEN, "testFiles", "fastq_subset*.fq")))
NEW_ENTRY_POINTS = ["ts_chunk_reserve", "ts_chunk_upload", "ts_fastq_chunk_walk", "ts_fastq_chunk_stage", "ts_fastq_chunk_gather"]


def golden_runs():
    """(manifest name, flags, input path, expected path or None, stdin?) of every --fastq-subset manifest that reads an
    uncompressed committed input and writes to stdout."""
    runs = []
    for path in sorted(glob.glob(os.path.join(H.GOLDEN, "validateFiles", "fastq_subset*.tst"))):
        m = H.load_manifest(path)
        if m["mode"] != "directive" or " -o " in m["command"]:
            continue
        d = {}
        for k, v in m["directives"]:
            d.setdefault(k, []).append(v)
        toks = shlex.split(m["command"])
        stdin = "<" in toks
        files = [t for t in toks if t.startswith("testFiles/")]
        flags, skip = [], False
        for t in toks:
            if skip or t == "<" or t.startswith("testFiles/") or t == "--fastq-subset":
                skip = False
                continue
            if t == "-j":
                skip = True
                continue
            flags.append(t)
        so = d.get("expect_stdout", ["ignore"])[0]
        runs.append((os.path.basename(path)[:-4], flags, H.golden_path(files[0]), None if so == "ignore" else H.golden_path(so),
                     stdin, int(d["expect_exit"][0])))
    return runs


RUNS = golden_runs()


def test_every_committed_input_is_covered():
    names = {os.path.basename(p) for p in INPUTS}
    assert {"fastq_subset_crlf.fq", "fastq_subset_blanklines.fq", "fastq_subset.fq", "fastq_subset_large.fq"} <= names
    used = {os.path.basename(r[2]) for r in RUNS}
    assert names <= used | {"fastq_subset.fq.gz"}, names - used


@pytest.mark.parametrize("path", INPUTS, ids=[os.path.basename(p) for p in INPUTS])
def test_walk_reproduces_the_file(path):
    """Offsets and sizes of the table give back the file's records and sequences as the line reader of tests/harness.py
    (readFastqRecord restated with split) finds them, and nothing but blank lines lies between them."""
    text = open(path, "rb").read()
    recs, nxt, err, _, _ = F.ref_walk(text, True)
    assert (nxt, err) == (len(text), F.OK)
    want = H.read_fastq_records(text)
    assert len(recs) == len(want) > 0
    end = 0
    for (off, seq_at, seq_len, size, seq_cr), (raw, seq) in zip(recs, want):
        assert text[end:off].replace(b"\r", b"").replace(b"\n", b"") == b"" and off >= end
        assert text[off:off + size] + b"\n" == raw
        assert text[off + seq_at:off + seq_at + seq_len] == seq
        assert seq_cr == (1 if seq.endswith(b"\r") else 0)
        end = off + size + 1
    assert text[end:].strip(b"\r\n") == b""
    # the same table from a text cut anywhere: what is not consumed is carried
    for cut in range(0, len(text), max(1, len(text) // 97)):
        head, nxt, err, _, _ = F.ref_walk(text[:cut], False)
        assert err == F.OK and head == recs[:len(head)] and nxt <= cut
        rest, nxt2, err2, _, _ = F.ref_walk(text[nxt:], True)
        assert err2 == F.OK and [(r[0] + nxt,) + r[1:] for r in rest] == recs[len(head):] and nxt + nxt2 == len(text)


@pytest.mark.parametrize("run", [r for r in RUNS if r[3]], ids=[r[0] for r in RUNS if r[3]])
def test_walk_and_oracle_filter_reproduce_the_expected_subset(run):
    _, flags, src, expected, _, _ = run
    text = open(src, "rb").read()
    if src.endswith(".gz"):
        text = gzip.decompress(text)
    opts = H.parse_cli("--fastq-subset " + " ".join(flags))
    out, kept, total = F.ref_subset(text, OracleReadFilter(opts))
    assert out == open(expected, "rb").read()
    assert total == len(H.read_fastq_records(text)) and 0 <= kept <= total


@pytest.mark.parametrize("name", sorted(F.edge_cases()))
def test_edge_cases_against_the_line_reader(name):
    text = F.edge_cases()[name]
    recs, nxt, err, _, _ = F.ref_walk(text, True)
    want = H.read_fastq_records(text)
    assert (nxt, err) == (len(text), F.OK) and len(recs) == len(want)
    for r, (raw, seq) in zip(recs, want):
        assert text[r[0]:r[0] + r[3]] + b"\n" == raw and text[r[0] + r[1]:r[0] + r[1] + r[2]] == seq
    opts = H.parse_cli("--fastq-subset -x 0 -l 18 -y 0.8 -k 10 -d 10")
    rf = OracleReadFilter(opts)
    assert F.ref_subset(text, rf) == H.run_fastq_subset(rf, text)


def test_edge_cases_hold_what_they_name():
    e = F.edge_cases()
    quals = [e["quality begins with @ and +"][r[0]:r[0] + r[3]].split(b"\n")[3][:1] for r in F.ref_walk(e["quality begins with @ and +"], True)[0]]
    assert b"@" in quals and b"+" in quals
    assert e["plus repeats the name"].count(b"\n+c\n") == 2
    assert [r[2] for r in F.ref_walk(e["empty sequence and quality"], True)[0]].count(0) == 2
    assert not e["no final newline"].endswith(b"\n") and e["no final newline, only the cr"].endswith(b"\r")
    assert b"\n\n\n@" in e["blank lines before headers"] and b"\r\n\r\n\n@" in e["blank lines before headers"]
    assert F.ref_walk(e["sequence of a lone cr"], True)[0][0][2:] == (1, 8, 1)
    gen = e["generated"]
    lines = gen.split(b"\n")
    assert b"" in lines[:-1] and b"\r" in lines and any(r[2] == 0 for r in F.ref_walk(gen, True)[0])


@pytest.mark.parametrize("name", sorted(F.error_cases()))
def test_error_cases(name):
    """Kind and record of the error, the records in front of it, and the host route's message through the line reader of
    tests/harness.py, which stops at the same record."""
    text, kind, at = F.error_cases()[name]
    recs, nxt, err, bad, off = F.ref_walk(text, True)
    assert (err, bad) == (kind, at) and len(recs) == at and nxt == off
    assert off == (recs[-1][0] + recs[-1][3] + 1 if recs else 0) or text[off - 1:off] == b"\n"
    with pytest.raises(ValueError) as ei:
        H.read_fastq_records(text)
    assert str(ei.value) == F.MESSAGES[kind]
    with pytest.raises(ValueError) as ei:
        F.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset -l 18")))
    assert str(ei.value) == "FASTQ record %d: %s" % (at + 1, F.MESSAGES[kind])
    # not at the end of the input, a truncated record is the carry and nothing is wrong
    if kind == F.TRUNCATED:
        head, nxt, err, _, _ = F.ref_walk(text, False)
        assert err == F.OK and head == recs and nxt == off


def test_error_cases_cover_every_kind_and_place():
    cases = F.error_cases()
    for kind in (F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS):
        places = {at for _, k, at in cases.values() if k == kind}
        assert len(places) >= 3
    assert any(k == F.TRUNCATED for _, k, _ in cases.values())
    assert "two errors: the lower one" in cases


def test_malformed_golden_input():
    text = open(H.golden_path("testFiles/fastq_malformed.fq"), "rb").read()
    assert F.ref_walk(text, True)[2:4] == (F.BAD_LENGTHS, 0)


def test_header_declares_and_library_exports_the_device_route():
    """Fails without the feature: include/teloscan.h declares the entry points of the device FASTQ route (each naming the
    reference lines it replaces), libteloscan.so exports them, and the record's mirror has the C compiler's size."""
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert "typedef struct ts_bam_chunk ts_chunk;" in bare
    for code in ("TS_FASTQ_OK", "TS_FASTQ_TRUNCATED", "TS_FASTQ_BAD_HEADER", "TS_FASTQ_BAD_SEPARATOR", "TS_FASTQ_BAD_LENGTHS"):
        assert re.search(r"#define\s+%s\s+\d" % code, bare), code
    for name in NEW_ENTRY_POINTS:
        comment = hdr[:hdr.index(name + "(")].rsplit("/*", 1)[1]
        assert "src/input.cpp:" in comment, name
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert lib.ts_abi_version() == 4
    assert C.sizeof(K.FastqRecord) == 24
    assert (K.FASTQ_OK, K.FASTQ_TRUNCATED, K.FASTQ_BAD_HEADER, K.FASTQ_BAD_SEPARATOR, K.FASTQ_BAD_LENGTHS) == \
        (F.OK, F.TRUNCATED, F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS)


def test_record_mirror_matches_the_c_struct(tmp_path):
    from teloscope_amd import _capi as K
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "teloscan.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(ts_fastq_record), offsetof(ts_fastq_record, off), offsetof(ts_fastq_record, seq_at), '
                   'offsetof(ts_fastq_record, seq_len), offsetof(ts_fastq_record, size), offsetof(ts_fastq_record, seq_cr));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = K.FastqRecord
    assert got == [C.sizeof(R), R.off.offset, R.seq_at.offset, R.seq_len.offset, R.size.offset, R.seq_cr.offset]


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fastq_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def test_cli_builds_and_refuses_without_a_device(tmp_path):
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    cli = build_cli(tmp_path / "fastq_device_cli")
    r = subprocess.run([cli, "-x", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--fastq-subset" in r.stderr
    if K.lib().ts_device_count() > 0:
        return                                                   # (with a device: tests/test_gpu_fastq_device.py)
    for route in ("--device", "--host"):
        r = subprocess.run([cli, "--fastq-subset", route, H.golden_path("testFiles/fastq_subset.fq")], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr and r.stdout == ""
