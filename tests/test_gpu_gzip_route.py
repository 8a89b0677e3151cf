"""The three text routes reading plain gzip on the device (detail::ChunkFeed's Gzip source), device route against host route of
the same binary, with TS_GZIP_DEVICE=1, TS_GZIP_MIN_BYTES=0 and TS_GZIP_SPAN=4096 set for the child processes so that the
small committed inputs take the new path: every committed FASTQ, FASTA and GFA input plain-gzipped, at the default chunk size
and in 4096-byte chunks; BGZF members followed by a plain gzip member cut inside a record; the six file classes (good,
truncated, wrong CRC, flipped bit, trailing garbage, two members) as FASTQ; and one run with TS_GZIP_DEVICE=0.  That the
device and not zlib produced the bytes is tests/test_gpu_gzip_feed.py's to show (the routes do not print the statistics)."""
import gzip

import pytest

from tests import fastqchunk as F
from tests import harness as H
from tests import test_gpu_fasta_device as FA
from tests import test_gpu_fastq_device as FQ
from tests import test_gpu_gfa_device as GF
from tests.backends import OracleReadFilter
from tests.test_bam_subset import EOF_BLOCK, bgzf
from tests.test_fasta_chunk_reference_cpu import INPUTS as FASTA_INPUTS
from tests.test_fasta_chunk_reference_cpu import build_cli as build_fasta
from tests.test_fastq_chunk_reference_cpu import INPUTS as FASTQ_INPUTS
from tests.test_fastq_chunk_reference_cpu import build_cli as build_fastq
from tests.test_gfa_chunk_reference_cpu import INPUTS as GFA_INPUTS
from tests.test_gfa_chunk_reference_cpu import build_cli as build_gfa

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def gzip_on_the_device(monkeypatch):
    monkeypatch.setenv("TS_GZIP_DEVICE", "1")
    monkeypatch.setenv("TS_GZIP_MIN_BYTES", "0")
    monkeypatch.setenv("TS_GZIP_SPAN", "4096")


@pytest.fixture(scope="module")
def clis(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    d = tmp_path_factory.mktemp("cpp")
    return {"fastq": build_fastq(d / "fastq_device_cli"), "fasta": build_fasta(d / "fasta_device_cli"), "gfa": build_gfa(d / "gfa_device_cli")}


def gzipped(tmp_path, paths, suffix):
    out = []
    for k, p in enumerate(paths):
        data = open(p, "rb").read()
        q = tmp_path / ("in%02d%s.gz" % (k, suffix))
        q.write_bytes(data if p.endswith(".gz") else gzip.compress(data, (1, 6, 9)[k % 3]))
        out.append(q)
    return out


@pytest.mark.parametrize("chunk", [None, 4096])
def test_every_committed_fastq_plain_gzipped(clis, tmp_path, chunk):
    assert len(FASTQ_INPUTS) >= 4
    for p in gzipped(tmp_path, FASTQ_INPUTS, ".fq"):
        text = gzip.decompress(p.read_bytes())
        plain = tmp_path / (p.name + ".plain.fq")
        plain.write_bytes(text)
        flags = ["-l", "18"] + (["--fastq-chunk-bytes", str(chunk)] if chunk else [])
        d, _ = FQ.both(clis["fastq"], flags, path=p)
        e, _ = FQ.both(clis["fastq"], flags, path=plain)
        assert d.returncode == e.returncode and d.stdout == e.stdout, p.name     # (gzipped == plain, good input or malformed)


@pytest.mark.parametrize("chunk", [None, 4096])
def test_every_committed_fasta_plain_gzipped(clis, tmp_path, chunk):
    inputs = gzipped(tmp_path, FASTA_INPUTS, ".fa")
    flags = FA.HEADLINE.split() + (["--chunk-bytes", str(chunk)] if chunk else [])
    d, _, files = FA.both(clis["fasta"], tmp_path, flags, inputs)
    assert d.returncode == 0, d.stderr[-300:]
    assert len([f for f in files if f.endswith("_report.tsv")]) == len(inputs)


@pytest.mark.parametrize("chunk", [None, 4096])
def test_every_committed_gfa_plain_gzipped(clis, tmp_path, chunk):
    inputs = gzipped(tmp_path, GFA_INPUTS, ".gfa")
    d, files = GF.both(clis["gfa"], tmp_path, ["--chunk-bytes", str(chunk)] if chunk else [], inputs)
    assert d.returncode == 0, d.stderr[-300:]
    assert len(files) == 2 * len(inputs)


@pytest.mark.parametrize("mix", ["eof_between", "no_eof", "trailing", "trailing_no_eof"])
def test_bgzf_members_then_plain_gzip(clis, tmp_path, mix):
    """The `mix` cases of tests/test_gpu_fastq_device.py, the plain gzip member now decoded on the device as well."""
    text = F.reads_text(71, 120, lo=30, hi=400)
    want, kept, total = F.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset -l 42")))
    cut = len(text) // 2 + 7
    members, whole = bgzf(text[:cut], 600), bgzf(text, 600)
    data = {"eof_between": members + gzip.compress(text[cut:], 6), "no_eof": members[:-len(EOF_BLOCK)] + gzip.compress(text[cut:], 6),
            "trailing": whole + b"not gzip at all\n", "trailing_no_eof": whole[:-len(EOF_BLOCK)] + b"xy"}[mix]
    p = tmp_path / (mix + ".fq.gz")
    p.write_bytes(data)
    for chunk in (["--fastq-chunk-bytes", "1000", "--reads-per-batch", "5"], ["--fastq-chunk-bytes", "4096"], []):
        d, _ = FQ.both(clis["fastq"], ["-l", "42"] + chunk, path=p, timeout=120)
        assert d.returncode == 0 and d.stdout == want, (mix, chunk, d.stderr[-300:])
        assert ("FASTQ subset: kept %d of %d reads." % (kept, total)).encode() in d.stderr


def test_the_six_file_classes_as_fastq(clis, tmp_path, monkeypatch):
    text = F.reads_text(5, 3000, lo=80, hi=250)
    other = F.reads_text(6, 500, lo=80, hi=250)
    good = gzip.compress(text, 6)
    flip = bytearray(good); flip[len(good) // 2] ^= 0x10
    crc = bytearray(good); crc[-6] ^= 1
    classes = {"good": (good, 0), "truncated": (good[:len(good) // 2], None), "wrong_crc": (bytes(crc), 1), "flipped_bit": (bytes(flip), 1),
               "trailing_garbage": (good + b"garbage that is no member" * 4, 0), "two_members": (good + gzip.compress(other, 9), 0)}
    for name, (data, rc) in classes.items():
        p = tmp_path / (name + ".fq.gz")
        p.write_bytes(data)
        for chunk in ([], ["--fastq-chunk-bytes", "4096"]):
            d, h = FQ.both(clis["fastq"], ["-l", "42"] + chunk, path=p, timeout=120)      # (same status, same message, same bytes on success)
            assert rc is None or d.returncode == rc, (name, d.stderr[-300:])
    # TS_GZIP_DEVICE=0: zlib as before, the same bytes
    p = tmp_path / "two_members.fq.gz"
    on, _ = FQ.both(clis["fastq"], ["-l", "42"], path=p)
    monkeypatch.setenv("TS_GZIP_DEVICE", "0")
    off, _ = FQ.both(clis["fastq"], ["-l", "42"], path=p)
    assert on.returncode == off.returncode == 0 and on.stdout == off.stdout and len(on.stdout) > 0
