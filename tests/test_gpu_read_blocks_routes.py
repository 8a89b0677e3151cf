"""The read block report through the six subset routes of include/teloscope_mi355x_io.hpp (tests/cpp/read_blocks_cli.cpp): the
device routes' report == the host routes' == tests/readblocks.py: ref_report on the CPU oracle, byte for byte, per front end, on a
tiled set and mixed_5_6, from a plain file, bgzip, gzip and stdin, at chunk sizes 4096 and 65536 with 37 reads per batch, on 1, 2
and 3 contexts, BAM with both walks and both deflate forms; the lines written before a bad record; and no formatter call without
--blocks."""
import gzip
import os
import re
import subprocess

import pytest

from tests import readblocks as B
from tests import readsets as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED = "-l 42"
FLAGS = [TILED, R.SETS[0]]
IDS = ["tiled", R.SET_IDS[0]]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from teloscope_amd import _capi
    _capi.lib()
    exe = tmp_path_factory.mktemp("read_blocks_cli") / "read_blocks_cli"
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "read_blocks_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(exe)])
    return str(exe)


def reads_of(flags):
    return [r for r in R.reads_for(flags) if r]


def inputs(kind, reads, d):
    """-> ({label: the line of an --each list}, names)"""
    if kind == "bam":
        data, names = B.bam_file(reads, 3000)
        files = {"file": data, "stdin": data}
    else:
        text, names = (B.fastq_input if kind == "fastq" else B.sam_input)(reads)
        files = {"plain": text, "bgzip": B.bgzf(text, 5000), "gzip": gzip.compress(text), "stdin": text}
    lines = {}
    for label, data in files.items():
        path = d / ("in_" + label)
        path.write_bytes(data)
        lines[label] = ("<" if label == "stdin" else "") + str(path)
    return lines, names


def run_each(cli, kind, flags, d, lines, extra):
    """one process over every input of `lines` -> {label: (blocks bytes, the .ok line)}, stderr"""
    for line in lines.values():
        for suffix in (".out", ".ok", ".err", ".partial", ".blocks"):
            if os.path.exists(line.lstrip("<") + suffix):
                os.remove(line.lstrip("<") + suffix)
    listing = d / "list"
    listing.write_text("".join(ln + "\n" for ln in lines.values()))
    p = subprocess.run([cli, "--%s-subset" % kind, "--each", str(listing), "--reads-per-batch", "37"] + extra + flags.split(),
                       stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    got = {}
    for label, line in lines.items():
        path = line.lstrip("<")
        assert os.path.exists(path + ".ok"), (label, open(path + ".err").read() if os.path.exists(path + ".err") else p.stderr)
        got[label] = (open(path + ".blocks", "rb").read() if os.path.exists(path + ".blocks") else None, open(path + ".ok").read())
    return got, p.stderr.decode(errors="replace")


DEVICE_RUNS = [["--contexts", "1", "--chunk-bytes", "4096"], ["--contexts", "2", "--chunk-bytes", "65536"],
               ["--contexts", "3", "--chunk-bytes", "4096"], ["--contexts", "1", "--chunk-bytes", "65536"]]
BAM_FORMS = [["--bam-walk", "serial", "--bam-deflate", "host"], ["--bam-walk", "index", "--bam-deflate", "device"],
             ["--bam-walk", "serial", "--bam-deflate", "device"], ["--bam-walk", "index", "--bam-deflate", "host"]]


@pytest.mark.parametrize("kind", ["fastq", "sam", "bam"])
@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
def test_device_equals_host_equals_reference(cli, tmp_path, flags, kind):
    reads = reads_of(flags)
    lines, names = inputs(kind, reads, tmp_path)
    exp, kept = B.ref_report(list(zip(names, reads)), B.read_oracle(flags))
    assert exp and 0 < len(kept) < len(reads)
    n_lines = exp.count(b"\n")
    ok = "read subset: kept %d of %d records, %d block lines.\n" % (len(kept), len(reads), n_lines)
    # the names in the report are the kept names, in order
    named = []
    for ln in exp.splitlines():
        if not named or named[-1] != ln.split(b"\t")[0]:
            named.append(ln.split(b"\t")[0])
    assert named == kept
    runs = [["--host", "--blocks", "-"]] + [["--device", "--blocks", "-"] + r + (BAM_FORMS[i] if kind == "bam" else []) for i, r in enumerate(DEVICE_RUNS)]
    for extra in runs:
        got, _ = run_each(cli, kind, flags, tmp_path, lines, extra + ["--stats"])
        for label, (blocks, figures) in got.items():
            assert blocks == exp, (extra, label)
            assert figures == ok, (extra, label)


def test_without_blocks_nothing_is_formatted(cli, tmp_path):
    reads = reads_of(TILED)
    for kind in ("fastq", "sam", "bam"):
        lines, _ = inputs(kind, reads, tmp_path)
        one = {k: v for k, v in lines.items() if k in ("plain", "file")}
        with_report, err = run_each(cli, kind, TILED, tmp_path, one, ["--device", "--blocks", "-", "--stats"])
        m = re.search(r"read block text: (\d+) calls, (\d+) lines, (\d+) bytes", err)
        blocks = list(with_report.values())[0][0]
        assert m and int(m.group(1)) > 0 and int(m.group(2)) == blocks.count(b"\n") and int(m.group(3)) == len(blocks)
        subset = open(list(one.values())[0] + ".out", "rb").read()
        without, err = run_each(cli, kind, TILED, tmp_path, one, ["--device", "--stats"])
        assert "read block text: 0 calls, 0 lines, 0 bytes" in err
        assert list(without.values())[0][0] is None
        assert open(list(one.values())[0] + ".out", "rb").read() == subset       # the subset's bytes do not depend on the report
        assert list(without.values())[0][1].endswith(", 0 block lines.\n")


@pytest.mark.parametrize("kind,routes", [("sam", ["--host", "--device"]), ("fastq", ["--device"])])
def test_lines_before_a_bad_record_in_the_second_chunk(cli, tmp_path, kind, routes):
    """The bad record lies behind the first 65536 bytes; the report holds exactly the lines of the records written before the
    message.  (fastqSubset, the host route, stops its batch at the bad record and writes none of it: only its device route keeps
    the valid records of the chunk, as it does for the subset itself.)"""
    reads = reads_of(TILED)
    build = B.fastq_input if kind == "fastq" else B.sam_input
    text, names = build(reads)
    # cut the input behind whole records, some 70 000 bytes in
    sizes, good = [], 0
    for i in range(len(reads)):
        t, _ = build(reads[:i + 1])
        sizes.append(len(t))
        if len(t) > 70_000:
            good = i + 1
            break
    assert good and sizes[-1] > 65_536
    head, _ = build(reads[:good])
    bad = b"@bad\nACGT\n-\nIIII\n" if kind == "fastq" else b"bad\t4\t*\n"
    path = tmp_path / "bad_input"
    path.write_bytes(head + bad + text[len(head):])
    exp, kept = B.ref_report(list(zip(names[:good], reads[:good])), B.read_oracle(TILED))
    assert exp
    for route in routes:
        for suffix in (".out", ".ok", ".err", ".partial", ".blocks"):
            if os.path.exists(str(path) + suffix):
                os.remove(str(path) + suffix)
        listing = tmp_path / "list"
        listing.write_text(str(path) + "\n")
        p = subprocess.run([cli, "--%s-subset" % kind, route, "--each", str(listing), "--blocks", "-", "--reads-per-batch", "37", "--chunk-bytes", "65536"] +
                           TILED.split(), stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert os.path.exists(str(path) + ".err") and not os.path.exists(str(path) + ".ok")
        message = open(str(path) + ".err").read()
        assert ("FASTQ record %d" % (good + 1) if kind == "fastq" else "SAM line %d" % (good + 1)) in message, message
        assert open(str(path) + ".blocks", "rb").read() == exp, route
        partial = open(str(path) + ".partial", "rb").read()
        assert partial.count(b"\n") == (4 if kind == "fastq" else 1) * len(kept)
