"""Without a device: the plain-Python FASTA references of tests/fastachunk.py (what tests/test_gpu_fasta_chunk.py holds the
device stages against) pinned by the host reader — tests/cpp/fasta_device_cli.cpp --dump-records prints FastaGroupReader's
view of a file — on every committed FASTA input and on the generators' edge cases, and by the committed *_gaps.bed files; the
C-ABI of the device stages and TS_INPUT_DEVICE declared and exported; the test program builds and refuses to run without a
device."""
import ctypes as C
import glob
import gzip
import os
import re
import subprocess

import pytest

from tests import fastachunk as F
from tests import harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = sorted(glob.glob(os.path.join(H.GOLDEN, "testFiles", "*.fa")) + glob.glob(os.path.join(H.GOLDEN, "testFiles", "*.fa.gz")))
GAP_BEDS = sorted(glob.glob(os.path.join(H.GOLDEN, "testFiles", "expected", "*_gaps.bed")))
NEW_ENTRY_POINTS = ["ts_fasta_chunk_walk", "ts_fasta_chunk_join", "ts_fasta_chunk_runs", "ts_fasta_chunk_bases"]


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fasta_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("fasta_cli") / "fasta_device_cli")


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for c in data:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def reference_dump(text):
    """The reference's view of a complete text, in the form --dump-records prints."""
    recs, nxt, names = F.ref_walk(text, True)
    assert nxt == len(text)
    lines = []
    for r in recs:
        bases = F.ref_bases(text, r)
        assert len(bases) == r[3]
        runs = ",".join("%s:%d:%d" % ("G" if g else "S", s, n) for g, s, n in F.ref_runs_of(bases))
        lines.append(b"%s\t%d\t%016x\t%s" % (F.name_word(names[r[4]:r[4] + r[5]]), len(bases), fnv1a64(bases), runs.encode()))
    return lines


def host_dump(cli, path):
    r = subprocess.run([cli, "--dump-records", str(path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.split(b"\n")[:-1]


def test_inputs_are_there():
    names = {os.path.basename(p) for p in INPUTS}
    assert len(INPUTS) >= 30 and {"multi.fa", "bTaeGut7_chr33_mat.fa.gz", "bTaeGut7_chr33_pat.fa.gz"} <= names
    assert len(GAP_BEDS) >= 10


@pytest.mark.parametrize("path", [p for p in INPUTS if not p.endswith(".gz")], ids=lambda p: os.path.basename(p))
def test_reference_equals_host_reader_on_committed_fasta(cli, path):
    text = open(path, "rb").read()
    assert reference_dump(text) == host_dump(cli, path)
    # the same table from a text cut anywhere: what is not consumed is carried
    whole = F.ref_walk(text, True)[0]
    for cut in range(0, len(text), max(1, len(text) // 23)):
        head, nxt, _ = F.ref_walk(text[:cut], False)
        assert [r[:4] for r in head] == [r[:4] for r in whole[:len(head)]] and nxt <= cut
        rest, nxt2, _ = F.ref_walk(text[nxt:], True)
        assert [(r[0] + nxt,) + r[1:4] for r in rest] == [r[:4] for r in whole[len(head):]] and nxt + nxt2 == len(text)


@pytest.mark.parametrize("path", [p for p in INPUTS if p.endswith(".gz")], ids=lambda p: os.path.basename(p))
def test_reference_equals_host_reader_on_the_compressed_chromosomes(cli, path):
    """The two real chromosomes (4 Mb each): name, base count, the hash of the bases and every run.  The runs come from a
    regular expression over the reference's bases, so that the byte loop of ref_runs_of does not run over megabases."""
    text = gzip.decompress(open(path, "rb").read())
    recs, nxt, names = F.ref_walk(text, True)
    got = host_dump(cli, path)
    assert nxt == len(text) and len(recs) == len(got) == 1
    name, n, fnv, runs = got[0].split(b"\t")
    bases = F.ref_bases(text, recs[0])
    assert len(bases) == recs[0][3]
    assert (name, int(n), fnv) == (F.name_word(names), len(bases), b"%016x" % fnv1a64(bases))
    want, at = [], 0
    for m in re.finditer(b"[NnXx]+", bases):
        if m.start() > at:
            want.append(b"S:%d:%d" % (at, m.start() - at))
        want.append(b"G:%d:%d" % (m.start(), m.end() - m.start()))
        at = m.end()
    if at < len(bases):
        want.append(b"S:%d:%d" % (at, len(bases) - at))
    assert runs.split(b",") == want


@pytest.mark.parametrize("name", sorted(F.edge_cases()))
def test_reference_equals_host_reader_on_edge_cases(cli, tmp_path, name):
    text = F.edge_cases()[name]
    path = tmp_path / "case.fa"
    path.write_bytes(text)
    assert reference_dump(text) == host_dump(cli, path), name
    # through zlib (the reader's other parser) the view is the same — but for a header line that the input ends in without a
    # newline, which that parser never completes; the references follow the parser of mapped files, which keeps the record
    gz = tmp_path / "case.fa.gz"
    gz.write_bytes(gzip.compress(text))
    want = host_dump(cli, path)
    assert host_dump(cli, gz) == (want[:-1] if name.startswith("header with") else want), name


@pytest.mark.parametrize("bed", GAP_BEDS, ids=lambda p: os.path.basename(p))
def test_reference_runs_reproduce_the_golden_gap_beds(bed):
    fasta = H.golden_path("testFiles/" + os.path.basename(bed)[:-len("_gaps.bed")])
    text = open(fasta, "rb").read()
    recs, _, names = F.ref_walk(text, True)
    lines = []
    for i, is_gap, start, ln in F.ref_runs(text, recs):
        if is_gap:
            lines.append("%s\t%d\t%d" % (F.name_word(names[recs[i][4]:recs[i][4] + recs[i][5]]).decode(), start, start + ln))
    with open(bed) as fh:
        assert lines == [l.rstrip("\n") for l in fh if l.strip()]


def test_edge_cases_hold_what_they_name():
    e = F.edge_cases()
    walk = lambda k: F.ref_walk(e[k], True)
    assert [r[3] for r in walk("record with no body")[0]] == [0, 4, 0]
    assert [r[3] for r in walk("body of blank lines only")[0]] == [0, 4]
    assert len(walk("gt in mid-line")[0]) == 3 and F.ref_bases(e["gt in mid-line"], walk("gt in mid-line")[0][0]) == b"AC>GTA>"
    assert walk("text in front of the first header")[0][0][0] == 17
    assert walk("no header at all") == ([], 10, b"") and F.ref_walk(e["no header at all"] + b"AC", False)[1] == 10
    assert e["no final newline, final cr"].endswith(b"\r") and F.ref_bases(e["no final newline, final cr"], walk("no final newline, final cr")[0][1])[-1:] != b"\r"
    assert F.ref_bases(e["stray cr inside a line"], walk("stray cr inside a line")[0][0]) == b"AC\rGT\r\rANN"
    assert F.ref_bases(e["space is a base"], walk("space is a base")[0][0]) == b"AC GT  N N"
    assert [r[1:] for r in F.ref_runs(e["one gap"], walk("one gap")[0])] == [(1, 0, 32), (0, 0, 4)]
    assert [r[:2] for r in F.ref_runs(e["gaps at both ends of neighbours"], walk("gaps at both ends of neighbours")[0])] == \
        [(0, 1), (0, 0), (0, 1), (1, 1), (1, 0), (1, 1), (2, 1), (2, 0), (2, 1)]
    assert len(F.ref_runs(e["anan"], walk("anan")[0])) == 4601
    assert [F.name_word(n) for n in (b"n1 some words", b"n2\twith tab", b"", b" lead")] == [b"n1", b"n2", b"", b""]
    # an unfinished record is the carry; a chunk that holds nothing else gives n = 0, next = 0
    assert F.ref_walk(b">a\nACGT\n", False) == ([], 0, b"") and F.ref_walk(b"xx\n>a\nAC", False) == ([], 3, b"")


def test_header_declares_and_library_exports_the_device_stages():
    """Fails without the feature: include/teloscan.h declares TS_INPUT_DEVICE and the FASTA stages (naming the reference lines
    they stand in for), libteloscan.so exports them, and the ABI version has not moved."""
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert re.search(r"#define\s+TS_INPUT_DEVICE\s+3\b", bare) and K.TS_INPUT_DEVICE == 3
    assert "src/input.cpp:" in hdr[hdr.index("FASTA text in the same resident chunk"):hdr.index("typedef struct ts_fasta_record")]
    assert "include/teloscope.h:260" in hdr[hdr.index("input_format TS_INPUT_DEVICE"):hdr.index("typedef struct ts_packed_run")]
    assert "TS_INPUT_DEVICE" in hdr[hdr.index("1 if segments of this kind"):hdr.index("ts_takes_text_input(")]
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert lib.ts_abi_version() == 4
    assert (C.sizeof(K.FastaRecord), C.sizeof(K.FastaRun)) == (32, 16)


def test_record_mirrors_match_the_c_structs(tmp_path):
    from teloscope_amd import _capi as K
    fields = {"ts_fasta_record": (K.FastaRecord, ["off", "text_len", "body_at", "n_bases", "name_at", "name_len", "reserved"]),
              "ts_fasta_run": (K.FastaRun, ["record", "is_gap", "start", "len"])}
    body = "".join('printf("%%zu ", sizeof(%s));%s' % (t, "".join('printf("%%zu ", offsetof(%s, %s));' % (t, f) for f in fs))
                   for t, (_, fs) in sorted(fields.items()))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "teloscan.h"\nint main(void){%s return 0;}' % body)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for t, (R, fs) in sorted(fields.items()):
        want += [C.sizeof(R)] + [getattr(R, f).offset for f in fs]
    assert got == want


def test_cli_refuses_without_a_device(cli):
    from teloscope_amd import _capi as K
    r = subprocess.run([cli, "-w", "1000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--device" in r.stderr and "--dump-records" in r.stderr
    if K.lib().ts_device_count() > 0:
        return                                                   # (with a device: tests/test_gpu_fasta_device.py)
    for route in ("--device", "--host"):
        r = subprocess.run([cli, route, H.golden_path("testFiles/multi.fa")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr and r.stdout == ""
