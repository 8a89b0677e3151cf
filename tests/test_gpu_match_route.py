"""The assembly scan's device route with the match files formatted on the device (scanFastaToFilesDevice, deviceTracks = true,
-m) through tests/cpp/match_text_cli.cpp: --device-tracks and --device against --host of the same binary on the committed FASTAs
— the same exit status, byte-equal console and byte-equal output files, every one of them — on plain and bgzipped input, in
4 KiB chunks, and with a record selector.  Under --device-tracks the library's counters must show the match lines formatted on
the device, as many as the two files hold, and the route must read no base back.  The formatter by itself:
tests/test_gpu_match_text.py; the scan entry point: tests/test_gpu_scan_match_text.py."""
import os
import re
import shlex
import subprocess

import pytest

from tests import harness as H
from tests import matchtext as M
from tests.test_bam_subset import bgzf
from tests.test_fasta_chunk_reference_cpu import INPUTS
from tests.test_gpu_fasta_device import files_of

pytestmark = pytest.mark.gpu

FLAG_SETS = ["-m", "-r -g -e -m -i", "-m -t 300 -n"]
PLAIN = [p for p in INPUTS if not p.endswith(".gz")]


@pytest.fixture(scope="module")
def mcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return M.build_match_cli(tmp_path_factory.mktemp("cpp") / "match_text_cli")


@pytest.fixture(scope="module")
def bgzipped(tmp_path_factory):
    """every plain committed FASTA, bgzipped in members of 3000 bytes of text (same file names, another directory)"""
    d = tmp_path_factory.mktemp("bgzf")
    out = []
    for p in PLAIN:
        q = d / (os.path.basename(p) + ".gz")
        q.write_bytes(bgzf(open(p, "rb").read(), 3000))
        out.append(str(q))
    return out


def run(mcli, out, route, flags, inputs, extra=()):
    lst = out.parent / (out.name + ".list")
    lst.write_text("".join(str(p) + "\n" for p in inputs))
    r = subprocess.run([mcli, route, "-o", str(out)] + shlex.split(flags) + list(extra) + ["--each", str(lst)], stdin=subprocess.DEVNULL,
                       capture_output=True, timeout=300)
    return r, files_of(out)


def stderr_numbers(r):
    err = r.stderr.decode(errors="replace")
    m = re.search(r"^match_text_stats (\d+) (\d+) (\d+) (\d+)$", err, re.M)
    u = re.search(r"^upload_stats((?: \d+){8})$", err, re.M)
    t = re.search(r"^route timing: read [\d.]+ ms scan [\d.]+ ms write [\d.]+ ms, bases read back (\d+) bytes$", err, re.M)
    assert m and u and t, err[-2000:]
    return [int(x) for x in m.groups()], [int(x) for x in u.group(1).split()], int(t.group(1))


def same(d, dfiles, h, hfiles):
    assert d.returncode == h.returncode == 0, (d.returncode, h.returncode, d.stderr[-400:], h.stderr[-400:])
    assert d.stdout == h.stdout
    assert sorted(dfiles) == sorted(hfiles)
    for name in hfiles:
        assert dfiles[name] == hfiles[name], name


def match_lines(files):
    return [sum(files[f].count(b"\n") for f in files if f.endswith(sfx)) for sfx in M.SUFFIXES]


def on_the_device(d, dfiles):
    """the counters of a --device-tracks run: every line of the two files was formatted on the device, no base came back"""
    stats, _, read_back = stderr_numbers(d)
    lines = match_lines(dfiles)
    assert lines[0] > 100
    assert stats[0] > 0 and stats[1:3] == lines, (stats, lines)
    assert stats[3] == sum(len(dfiles[f]) for f in dfiles if f.endswith(M.SUFFIXES))
    assert read_back == 0


@pytest.mark.parametrize("form", ["plain", "bgzip"])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_device_match_files_equal_the_host_route(mcli, bgzipped, tmp_path, flags, form):
    assert len(PLAIN) >= 30
    inputs = INPUTS if form == "plain" else bgzipped               # (the committed files as they are, two of them gzipped)
    h, hfiles = run(mcli, tmp_path / "host", "--host", flags, inputs)
    d, dfiles = run(mcli, tmp_path / "dev", "--device-tracks", flags, inputs)
    same(d, dfiles, h, hfiles)
    on_the_device(d, dfiles)
    assert stderr_numbers(h)[0] == [0, 0, 0, 0]
    # the device route without the flag: the same files, formatted on the host from bases it read back
    p, pfiles = run(mcli, tmp_path / "devhost", "--device", flags, inputs)
    same(p, pfiles, h, hfiles)
    stats, _, read_back = stderr_numbers(p)
    assert stats == [0, 0, 0, 0] and read_back > 0


def test_a_file_across_several_chunks(mcli, tmp_path):
    """4 KiB chunks: every larger FASTA spans several, and every chunk's lines are appended to the same two files."""
    flags = "-r -g -e -m -i"
    h, hfiles = run(mcli, tmp_path / "host", "--host", flags, PLAIN)
    d, dfiles = run(mcli, tmp_path / "dev", "--device-tracks", flags, PLAIN, ["--chunk-bytes", "4096"])
    same(d, dfiles, h, hfiles)
    on_the_device(d, dfiles)
    assert stderr_numbers(d)[0][0] > len(PLAIN)                      # more formatting calls than files


def test_with_a_record_selector(mcli, tmp_path):
    """--include-prefix on multi.fa: the record-filter overload of the device route formats the kept records' lines."""
    multi = H.golden_path("testFiles/multi.fa")
    first = open(multi).readline()[1:].split()[0]
    flags = "-r -g -e -m -i"
    extra = ["--include-prefix", first[:max(1, len(first) - 1)]]
    h, hfiles = run(mcli, tmp_path / "host", "--host", flags, [multi], extra)
    d, dfiles = run(mcli, tmp_path / "dev", "--device-tracks", flags, [multi], extra)
    same(d, dfiles, h, hfiles)
    stats, _, read_back = stderr_numbers(d)
    lines = match_lines(dfiles)
    assert stats[0] > 0 and stats[1:3] == lines and lines[0] > 0 and read_back == 0
    everything, _ = run(mcli, tmp_path / "all", "--device-tracks", flags, [multi])[1], None
    assert match_lines(everything)[0] > lines[0]                     # the selector dropped records that have matches
