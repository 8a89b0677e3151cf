"""The device route of the assembly scan (scanFastaToFilesDevice: FASTA text inflated, indexed, joined and cut at its N-runs on
the GPU, every segment scanned from device memory) through tests/cpp/fasta_device_cli.cpp: --device against --host of the same
binary on the same inputs — the same exit status, byte-equal stdout and byte-equal output files, every one of them.  The stages
are compared one by one with plain references in tests/test_gpu_fasta_chunk.py, TS_INPUT_DEVICE in
tests/test_gpu_input_device.py.  Every process is one bounded step."""
import glob
import gzip
import os
import random
import shlex
import subprocess

import pytest

from tests import fastachunk as F
from tests import harness as H
from tests.test_bam_subset import EOF_BLOCK, bgzf, bgzf_fancy
from tests.test_fasta_chunk_reference_cpu import INPUTS, build_cli
from tests.test_gpu_parity import WIDE_GRID

pytestmark = pytest.mark.gpu

HEADLINE = "-w 1000 -s 500 -r -g -e -m -i"
FLAG_SETS = {
    "headline": HEADLINE,
    "headline without -m": "-w 1000 -s 500 -r -g -e -i",
    "defaults": "",
    "tips only": "-u",
    "list form": "-p TTAGGG,TTAGG " + HEADLINE,
    "wide form": WIDE_GRID[1],
}


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "fasta_device_cli")


def files_of(d):
    return {os.path.basename(p): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(str(d), "*")))}


def both(dcli, tmp_path, flags, inputs, tag="run", timeout=300, extra_device=()):
    """The device run and the host run of the same command over `inputs` (one path, or a list through --each): equal exit
    status, byte-equal stdout and output files; -> (device result, host result, the device run's files)."""
    res, outs = [], []
    for route in ("--device", "--host"):
        out = tmp_path / ("%s%s" % (tag, route))
        cmd = [dcli, route, "-o", str(out)] + list(flags) + (list(extra_device) if route == "--device" else [])
        if isinstance(inputs, (list, tuple)):
            lst = tmp_path / (tag + ".list")
            lst.write_text("".join(str(p) + "\n" for p in inputs))
            cmd += ["--each", str(lst)]
        else:
            cmd.append(str(inputs))
        res.append(subprocess.run(cmd, stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout))
        outs.append(files_of(out))
    d, h = res
    assert d.returncode in (0, 1) and h.returncode in (0, 1), (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.returncode == h.returncode, (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.stdout == h.stdout
    assert sorted(outs[0]) == sorted(outs[1])
    for name in outs[1]:
        assert outs[0][name] == outs[1][name], name
    return d, h, outs[0]


@pytest.mark.parametrize("name", sorted(FLAG_SETS))
def test_every_committed_fasta(dcli, tmp_path, name):
    """All committed .fa files and the two .fa.gz as they lie, through one Teloscope per route."""
    assert len(INPUTS) >= 30
    d, _, files = both(dcli, tmp_path, shlex.split(FLAG_SETS[name]), INPUTS)
    assert d.returncode == 0, d.stderr[-300:]
    assert len([f for f in files if f.endswith("_report.tsv")]) == len(INPUTS)
    assert d.stdout.count(b"+++ Assembly Summary Report +++") == len(INPUTS)
    # (the wide set's patterns, TTA + A..., call no telomere on these assemblies)
    assert name == "wide form" or any(f.endswith("_terminal_telomeres.bed") and files[f] for f in files)
    if "-m" in FLAG_SETS[name]:
        assert any(f.endswith("_canonical_matches.bed") and files[f] for f in files)


def encodings(tmp_path, tag, text):
    """The text as a plain file, bgzipped, bgzipped and then plain-gzipped, plain-gzipped, with CRLF line ends and lower-cased."""
    half = len(text) // 2
    half = text.index(b"\n", half) + 1 if b"\n" in text[half:] else half
    out = []
    for name, data in (("plain", text), ("bgzf", bgzf_fancy(text, 1777, random.Random(5))),
                       ("bgzf_then_gzip", bgzf(text[:half], 3000)[:-len(EOF_BLOCK)] + gzip.compress(text[half:], 1)),
                       ("gzip", gzip.compress(text, 6)), ("crlf", text.replace(b"\n", b"\r\n")), ("lower", text.lower())):
        p = tmp_path / ("%s.%s.fa" % (tag, name))
        p.write_bytes(data)
        out.append(p)
    return out


def test_a_dozen_files_in_every_encoding(dcli, tmp_path):
    plain = [p for p in INPUTS if not p.endswith(".gz")]
    picked = [p for p in plain if os.path.basename(p).startswith(("gapped_", "multi"))][:8] + plain[:4]
    assert len(set(picked)) == 12
    inputs = []
    for k, p in enumerate(sorted(set(picked))):
        inputs += encodings(tmp_path, "f%02d" % k, open(p, "rb").read())
    d, _, files = both(dcli, tmp_path, shlex.split(HEADLINE) + ["--chunk-bytes", "4096"], inputs)
    assert d.returncode == 0, d.stderr[-300:]
    # every encoding of a file gives that file's outputs (lower case and CRLF too: the library folds case, line ends are no bases)
    for k in range(12):
        want = None
        for i in range(6 * k, 6 * k + 6):
            stem = "%d.%s" % (i, os.path.basename(str(inputs[i])))
            got = {f[len(stem):]: v for f, v in files.items() if f.startswith(stem + "_") and not f.endswith("_report.tsv")}
            assert len(got) >= 9
            want = got if want is None else want
            assert got == want, stem


@pytest.mark.parametrize("chunk", [1000, 65536, 1 << 20])
def test_chunk_sizes(dcli, tmp_path, chunk):
    """A multi-record file and a generated assembly of 120 records through chunks smaller than a record, of a few records and of
    everything at once: the chunks' carry, growth and record numbering."""
    gen = tmp_path / "generated.fa"
    gen.write_bytes(F.assembly_text(9, 120, hi=6000) + F.record_text(b"telomeric", b"CCCTAA" * 400 + F.random_bases(random.Random(1), 5000)
                                                                      + b"N" * 30 + b"TTAGGG" * 400, 80))
    d, _, files = both(dcli, tmp_path, shlex.split(HEADLINE) + ["--chunk-bytes", str(chunk)], [H.golden_path("testFiles/multi.fa"), gen])
    assert d.returncode == 0, d.stderr[-300:]
    assert files["1.generated.fa_gaps.bed"].count(b"\n") > 50 and b"telomeric" in files["1.generated.fa_terminal_telomeres.bed"]


def test_empty_file_and_file_without_a_record(dcli, tmp_path):
    for name, text in (("empty.fa", b""), ("no_record.fa", b"ACGT\nACGT\n"), ("only_blank.fa", b"\n\n")):
        p = tmp_path / name
        p.write_bytes(text)
        d, h, files = both(dcli, tmp_path, shlex.split(HEADLINE), p, tag=name)
        assert d.returncode == 0 and b"Total paths:\t0" in d.stdout, (name, d.stderr[-300:])


def test_damaged_bgzf_is_an_error_not_a_signal(dcli, tmp_path):
    """A flipped payload bit and a wrong CRC in a bgzipped assembly: the device run exits 1 with the BAM route's message."""
    text = F.assembly_text(12, 20)
    good = bytearray(bgzf(text, 3000))
    flipped = bytearray(good)
    flipped[18 + 40] ^= 0x10                                        # inside the first member's deflate payload
    first_total = int.from_bytes(good[16:18], "little") + 1
    crc = bytearray(good)
    crc[first_total - 8] ^= 0xff                                    # the first member's CRC32
    for name, data, msgs in (("flipped", flipped, (b"invalid BGZF deflate payload", b"BGZF checksum mismatch")), ("crc", crc, (b"BGZF checksum mismatch",))):
        p = tmp_path / (name + ".fa.gz")
        p.write_bytes(bytes(data))
        r = subprocess.run([dcli, "--device", "-o", str(tmp_path / name), str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and r.stderr[7:].strip() in msgs, (name, r.returncode, r.stderr[-200:])


def test_limits_are_refused_by_name(dcli, tmp_path):
    """Several devices (two contexts on this one GPU are several, as far as the route can tell) and a record that does not fit
    the largest chunk allowed (here 5 000 bytes instead of 4 GiB - 2): errors that say so, never a cut record."""
    multi = H.golden_path("testFiles/multi.fa")
    r = subprocess.run([dcli, "--device", "--devices", "0,0", "-o", str(tmp_path / "two"), multi], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"runs on one device" in r.stderr and b"made over 2" in r.stderr, r.stderr[-300:]
    r = subprocess.run([dcli, "--host", "--devices", "0,0", "-o", str(tmp_path / "two_host"), multi], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]
    p = tmp_path / "big_record.fa"
    p.write_bytes(F.record_text(b"small", b"ACGT" * 100) + F.record_text(b"too_big some words", b"ACGT" * 2500) + F.record_text(b"after", b"ACGT" * 10))
    for flags in ([], ["--chunk-bytes", "700"]):
        r = subprocess.run([dcli, "--device", "--chunk-limit", "5000", "-o", str(tmp_path / "big"), str(p)] + flags, stdin=subprocess.DEVNULL,
                           capture_output=True, timeout=120)
        assert r.returncode == 1 and b"FASTA record 'too_big' does not fit a device chunk" in r.stderr, r.stderr[-300:]
    d, _, _ = both(dcli, tmp_path, ["--chunk-bytes", "700"], p, tag="fits", extra_device=["--chunk-limit", "20000"])
    assert d.returncode == 0
