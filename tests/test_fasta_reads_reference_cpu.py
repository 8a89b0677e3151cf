"""Without a device: the plain-Python statement of the FASTA read subset (tests/fastareads.py, on tests/fastachunk.py's ref_walk:
what tests/test_gpu_fasta_reads_chunk.py and tests/test_gpu_fasta_reads_device.py hold the device against) pinned by the host
route's framing (tests/cpp/fasta_subset_cli.cpp --dump-records: detail::fastaWalkHost of include/teloscope_mi355x_reads_host.hpp)
on every committed FASTA input and on the rule's edge cases, with LF and with CR LF line ends; the host route itself over a
stand-in judge in a stand-alone program under ASan + UBSan (tests/cpp/fasta_subset_host.cpp); the C-ABI of the device route
declared, exported and bound; and the committed fixtures shown to be a mixture under the CPU oracle's read filter."""
import ctypes as C
import glob
import gzip
import os
import re
import subprocess

import pytest

from tests import fastachunk as F
from tests import fastareads as R
from tests import harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = sorted(glob.glob(os.path.join(H.GOLDEN, "testFiles", "*.fa")) + glob.glob(os.path.join(H.GOLDEN, "testFiles", "*.fa.gz")))
NEW_ENTRY_POINTS = ["ts_fasta_chunk_stage", "ts_fasta_chunk_gather", "ts_fasta_chunk_block_lines"]


def read_input(path):
    data = open(path, "rb").read()
    return gzip.decompress(data) if path.endswith(".gz") else data


def all_cases():
    """name -> complete text: every edge case as it is and, where it holds no '\\r' yet, with CR LF line ends."""
    cases = dict(R.edge_cases())
    cases.update({"assembly case: " + k: v for k, v in F.edge_cases().items()})
    for name, text in list(cases.items()):
        if b"\r" not in text:
            cases[name + " (crlf)"] = text.replace(b"\n", b"\r\n")
    return cases


CASES = all_cases()


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fasta_subset_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("fasta_reads_cpu") / "fasta_subset_cli")


def host_walk(cli, path):
    """--dump-records -> (records as ref_walk's tuples, next)"""
    r = subprocess.run([cli, "--dump-records", str(path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    lines = [l.split() for l in r.stdout.decode().splitlines()]
    assert lines[-1][0] == "next" and all(l[0] == "record" for l in lines[:-1])
    return [tuple(int(x) for x in l[1:]) for l in lines[:-1]], int(lines[-1][1])


@pytest.mark.parametrize("path", INPUTS, ids=lambda p: os.path.basename(p))
def test_reference_framing_equals_the_host_route_on_committed_fasta(cli, tmp_path, path):
    text = read_input(path)
    for tag, t in (("lf", text), ("crlf", text.replace(b"\n", b"\r\n"))):
        assert tag == "lf" or b"\r" not in text
        p = tmp_path / (tag + ".fa")
        p.write_bytes(t)
        recs, nxt, _ = F.ref_walk(t, True)
        assert host_walk(cli, p) == (recs, nxt) and nxt == len(t) and recs


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_framing_equals_the_host_route_on_edge_cases(cli, tmp_path, name):
    p = tmp_path / "case.fa"
    p.write_bytes(CASES[name])
    recs, nxt, _ = F.ref_walk(CASES[name], True)
    assert host_walk(cli, p) == (recs, nxt)


def test_edge_cases_hold_what_they_name():
    e = R.edge_cases()
    walk = lambda name: F.ref_walk(e[name], True)[0]                # noqa: E731
    assert [r[3] for r in walk("a body of no lines")] == [0, 54, 0] and walk("a body of no lines")[0][2] == walk("a body of no lines")[0][1]
    assert [r[3] for r in walk("a body of blank lines only")] == [0, 54]
    assert not e["one line without newline at the end"].endswith(b"\n") and walk("one line without newline at the end")[1][3] == 54
    assert e["a cr as the input's last byte"].endswith(b"G\r") and walk("a cr as the input's last byte")[1][3] == 54
    assert walk("a cr and no bases at the end")[1][3] == 0
    assert len(walk("a gt inside a body line")) == 3 and walk("a gt inside a body line")[0][3] == 13 + 55
    assert [R.ref_name(e["names"], r) for r in walk("names")] == [b"", b"", b"n2", b"n3", b"L" * 300]
    assert walk("a header with cr alone at the end")[1][5] == 6 and walk("only a gt") == [(0, 1, 1, 0, 0, 0)]
    # the written form: verbatim, and a newline behind the last record only where it lacks one
    for name, text in e.items():
        recs = F.ref_walk(text, True)[0]
        out, kept = R.ref_gather(text, recs, [1] * len(recs))
        assert kept == len(recs) and out == (text if text.endswith(b"\n") else text + b"\n"), name


def test_host_route_under_asan_and_ubsan(tmp_path):
    """tests/cpp/fasta_subset_host.cpp: detail::fastaSubsetHost over a stand-in judge, every block size, plain and gzip, against a
    whole-text statement written in the program; the sanitizers must have nothing to say."""
    exe = tmp_path / "fasta_subset_host"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-pthread", os.path.join(ROOT, "tests", "cpp", "fasta_subset_host.cpp"), "-o", str(exe), "-lz"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-600:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == "ok"
    assert {"fasta-every-block", "fasta-small-texts", "fasta-first-byte", "fasta-failing-output"} <= set(r.stdout.split()), r.stdout


def test_header_declares_and_library_exports_the_device_route():
    """Fails without the feature: include/teloscan.h states the rule and declares the entry points, libteloscan.so exports
    them and the binding names them."""
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    for msg in (R.EMPTY, R.NO_HEADER):
        assert msg in hdr, msg
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert lib.ts_abi_version() == 4
    host = open(os.path.join(ROOT, "include", "teloscope_mi355x_reads_host.hpp")).read()
    device = open(os.path.join(ROOT, "include", "teloscope_mi355x_io.hpp")).read()
    assert "fastaSubsetHost" in host and "FastaSubsetStats" in host and "fastaSubsetDevice" in device and "FastaReadChunkSteps" in device


def test_committed_fixtures_are_a_mixture_under_the_oracle():
    """The committed FASTA inputs as reads under the CPU oracle's read filter with default flags: 46 records, of which 42 pass
    and 4 do not — so a route that keeps everything, or nothing, cannot pass the tests that use them."""
    from tests.backends import OracleReadFilter
    rf = OracleReadFilter(H.parse_cli("--fastq-subset"))
    total = kept = 0
    per_file = {}
    parts = []
    for path in INPUTS:
        text = read_input(path)
        parts.append(text if text.endswith(b"\n") else text + b"\n")
        out, stats, msg, _ = R.ref_subset(text, rf)
        assert msg is None, (path, msg)
        per_file[os.path.basename(path)] = (stats[1], stats[0])
        total += stats[0]
        kept += stats[1]
    print(sorted((k, v) for k, v in per_file.items() if v[0] != v[1]))
    assert (total, kept) == (46, 42)
    assert {k: v for k, v in per_file.items() if v[0] != v[1]} == {"multi.fa": (2, 3), "gapped_none.fa": (0, 1), "no_telo.fa": (0, 1), "short_contig.fa": (0, 1)}
    out, stats, msg, _ = R.ref_subset(b"".join(parts), rf)
    assert msg is None and stats[0] == 46 and 0 < stats[1] < stats[0]
