"""The device route of --fastq-subset (fastqSubsetDevice: lines indexed, records framed and validated, sequences staged and
passing records gathered on the GPU) through tests/cpp/fastq_device_cli.cpp: --device against --host of the same binary on the
same input — equal return code, byte-equal stdout, the same message when both fail — and against the committed expected
subsets and the CPU oracle's read filter.  The stages are compared one by one with plain references in
tests/test_gpu_fastq_chunk.py.  Every process is one bounded step."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from tests import fastqchunk as F
from tests import harness as H
from tests import seqgen
from tests.backends import OracleReadFilter
from tests.test_bam_subset import EOF_BLOCK, bgzf, bgzf_fancy
from tests.test_fastq_chunk_reference_cpu import RUNS, build_cli

pytestmark = pytest.mark.gpu
FLAGS = ["-x", "0", "-l", "18", "-y", "0.8", "-k", "10", "-d", "10"]


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "fastq_device_cli")


def both(dcli, args, path=None, stdin_path=None, timeout=300):
    """The device run and the host run of the same command: (device result, host result); equal return codes, equal stdout
    when both succeed, the same message when both fail."""
    res = []
    for route in ("--device", "--host"):
        cmd = [dcli, "--fastq-subset", route] + list(args) + ([str(path)] if path is not None else [])
        with open(stdin_path, "rb") if stdin_path else open(os.devnull, "rb") as fh:
            res.append(subprocess.run(cmd, stdin=fh, capture_output=True, timeout=timeout))
    d, h = res
    assert d.returncode in (0, 1) and h.returncode in (0, 1), (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.returncode == h.returncode, (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    if d.returncode == 0:
        assert d.stdout == h.stdout
        assert d.stderr.splitlines()[-1] == h.stderr.splitlines()[-1]        # kept K of T reads
    else:
        assert d.stderr.splitlines()[-1] == h.stderr.splitlines()[-1] and d.stderr.startswith(b"Error:")
    return d, h


def encodings(tmp_path, tag, text):
    """The text as a plain file, bgzipped two ways (small members: several per chunk) and plain-gzipped."""
    out = {}
    for name, data in (("plain", text), ("bgzf", bgzf(text, 3000)), ("bgzf_fancy", bgzf_fancy(text, 1777, random.Random(5))),
                       ("gzip", gzip.compress(text, 6))):
        p = tmp_path / ("%s.%s" % (tag, name))
        p.write_bytes(data)
        out[name] = p
    return out


GOOD = [r for r in RUNS if r[5] == 0 and not r[2].endswith(".gz")]


@pytest.mark.parametrize("run", GOOD, ids=[r[0] for r in GOOD])
def test_golden_inputs_every_source(dcli, tmp_path, run):
    """Every committed input with its manifest's flags: as a plain file, bgzipped by the tests' own writers, plain-gzipped
    and on stdin — device == host == the expected subset."""
    name, flags, src, expected, _, _ = run
    want = open(expected, "rb").read()
    text = open(src, "rb").read()
    files = encodings(tmp_path, name, text)
    small = ["--fastq-chunk-bytes", "1000", "--reads-per-batch", "3"]
    for kind, chunk in (("plain", []), ("plain", small), ("bgzf", small), ("bgzf_fancy", []), ("gzip", [])):
        d, _ = both(dcli, flags + chunk, path=files[kind])
        assert d.returncode == 0 and d.stdout == want, (kind, chunk, d.stderr[-300:])
    for kind in ("plain", "gzip"):                                  # stdin: read in blocks, zlib where it is gzip
        d, _ = both(dcli, flags + ["--fastq-chunk-bytes", "777"], stdin_path=files[kind])
        assert d.returncode == 0 and d.stdout == want, (kind, d.stderr[-300:])


def test_committed_gzip_input(dcli):
    d, _ = both(dcli, FLAGS, path=H.golden_path("testFiles/fastq_subset.fq.gz"))
    assert d.returncode == 0 and d.stdout == open(H.golden_path("testFiles/expected/fastq_subset.fq"), "rb").read()
    assert b"FASTQ subset: kept 2 of 4 reads." in d.stderr


def kept_prefix_ok(text, flags, stdout):
    """stdout is a prefix of the kept well-formed records in input order, cut at a record's end."""
    recs = F.ref_walk(text, True)[0]
    with_seq = [r for r in recs if r[2] > r[4]]
    opts = H.parse_cli("--fastq-subset " + " ".join(flags))
    passes = OracleReadFilter(opts).filter([F.ref_sequence(text, r) for r in with_seq]) if with_seq else []
    kept = [text[r[0]:r[0] + r[3]] + b"\n" for r, ok in zip(with_seq, passes) if ok]
    ends, total = {0}, 0
    for k in kept:
        total += len(k)
        ends.add(total)
    return b"".join(kept).startswith(stdout) and len(stdout) in ends


def malformed_cases():
    cases = dict(F.error_cases())
    cases["fastq_malformed.fq"] = (open(H.golden_path("testFiles/fastq_malformed.fq"), "rb").read(), F.BAD_LENGTHS, 0)
    return sorted(cases.items())


MALFORMED = malformed_cases()


@pytest.mark.parametrize("i", range(len(MALFORMED)), ids=[name.replace(" ", "_") for name, _ in MALFORMED])
def test_malformed_inputs_fail_alike(dcli, tmp_path, i):
    """Both routes fail with the same message, and what either wrote before is a prefix of the kept well-formed records.
    Every case as a plain file through small chunks; every sixth also through one chunk, bgzipped and plain-gzipped."""
    name, (text, kind, at) = MALFORMED[i]
    files = encodings(tmp_path, "bad%d" % i, text)
    small = ["--fastq-chunk-bytes", "200", "--reads-per-batch", "2"]
    routes = [("plain", small)] + ([("plain", []), ("bgzf", small), ("gzip", [])] if i % 6 == 0 else [])
    for enc, chunk in routes:
        d, h = both(dcli, ["-x", "0", "-l", "6"] + chunk, path=files[enc], timeout=120)
        assert d.returncode == 1, (name, enc)
        msg = "Error: FASTQ record %d: %s" % (at + 1, F.MESSAGES[kind])
        assert d.stderr.decode().splitlines()[-1] == msg == h.stderr.decode().splitlines()[-1], (name, enc, d.stderr)
        assert kept_prefix_ok(text, ["-x", "0", "-l", "6"], d.stdout), (name, enc)
        assert kept_prefix_ok(text, ["-x", "0", "-l", "6"], h.stdout), (name, enc)


def test_refused_inputs_fail_alike(dcli, tmp_path):
    for text, msg in ((b"", b"FASTQ input is empty"), (b"\n@a\nAC\n+\nII\n", b"FASTQ input must start with '@'"), (b"ACGT\n", b"must start with '@'")):
        p = tmp_path / "refused.fq"
        p.write_bytes(text)
        for kw in (dict(path=p), dict(stdin_path=p)):
            d, h = both(dcli, [], timeout=120, **kw)
            assert d.returncode == 1 and msg in d.stderr and msg in h.stderr and d.stdout == b""


@pytest.mark.parametrize("flags", ["", "-l 42", "-x 0 -l 18 -y 0.8 -k 10 -d 10"])
def test_generated_reads_against_the_oracle(dcli, tmp_path, flags):
    text = F.reads_text(31, 600, lo=30, hi=900) + F.reads_text(32, 200, lo=30, hi=500, eol=b"\r\n")
    opts = H.parse_cli("--fastq-subset " + flags)
    want, kept, total = F.ref_subset(text, OracleReadFilter(opts))
    assert 0 < kept < total == 800
    files = encodings(tmp_path, "gen", text)
    for kind, path in files.items():
        d, _ = both(dcli, flags.split() + ["--fastq-chunk-bytes", "65536"], path=path)
        assert d.returncode == 0 and d.stdout == want, kind
        assert ("FASTQ subset: kept %d of %d reads." % (kept, total)).encode() in d.stderr


@pytest.fixture(scope="module")
def sizes_case(tmp_path_factory):
    text = F.reads_text(41, 1500, lo=10, hi=700)
    want = F.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset -l 42")))[0]
    return want, encodings(tmp_path_factory.mktemp("sizes"), "sizes", text)


@pytest.mark.parametrize("size", [1000, 65536, 1 << 20])
def test_chunk_size_independence(dcli, sizes_case, size):
    want, files = sizes_case
    for kind in ("plain", "bgzf", "gzip"):
        d, _ = both(dcli, ["-l", "42", "--fastq-chunk-bytes", str(size), "--reads-per-batch", "97"], path=files[kind])
        assert d.returncode == 0 and d.stdout == want, (size, kind)
    d, _ = both(dcli, ["-l", "42", "--fastq-chunk-bytes", str(size), "--reads-per-batch", "97"], stdin_path=files["plain"])
    assert d.returncode == 0 and d.stdout == want, (size, "stdin")


def test_reads_larger_than_the_chunk(dcli, tmp_path):
    """A 1.4 Mb telomeric read and a 1.2 Mb plain read among short ones, through 1 MB chunks: the chunk grows."""
    rng = np.random.default_rng(123)
    gen = random.Random(6)
    big = bytearray(seqgen.random_dna(rng, 1_400_000).tobytes())
    t = seqgen.repeat_array("CCCTAA", 2000).tobytes()
    big[-len(t):] = t
    plain = seqgen.random_dna(rng, 1_200_000).tobytes()
    short = [F.record_text(b"s%d" % i, F.random_read(gen, 100 + i, telomeric=i % 3 == 0)) for i in range(300)]
    text = b"".join(short[:200]) + F.record_text(b"big_telomeric", bytes(big)) + b"".join(short[200:250]) + \
        F.record_text(b"big_plain", plain) + b"".join(short[250:])
    want, kept, total = F.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset")))
    assert b"@big_telomeric\n" in want and b"@big_plain\n" not in want and total == 302
    files = encodings(tmp_path, "big", text)
    for kind in ("plain", "bgzf_fancy", "gzip"):
        d, _ = both(dcli, ["--fastq-chunk-bytes", str(1 << 20), "--reads-per-batch", "97"], path=files[kind])
        assert d.returncode == 0 and d.stdout == want, (kind, d.stderr[-300:])
    d, _ = both(dcli, ["--fastq-chunk-bytes", str(1 << 20)], stdin_path=files["plain"])
    assert d.returncode == 0 and d.stdout == want


def test_short_reads(dcli, tmp_path):
    """20 000 reads of 100-300 bases: the many-records case."""
    rng = np.random.default_rng(31)
    recs = []
    for i in range(20000):
        n = int(rng.integers(100, 301))
        s = seqgen.random_dna(rng, n).tobytes()
        if i % 50 == 0:
            s = (b"TTAGGG" * 60)[:n]
        recs.append(F.record_text(b"s%d" % i, s))
    text = b"".join(recs)
    files = encodings(tmp_path, "short", text)
    for kind in ("plain", "bgzf"):
        d, _ = both(dcli, ["-l", "42"], path=files[kind])
        assert d.returncode == 0, d.stderr[-300:]
        names = [l for l in d.stdout.split(b"\n")[0::4] if l]
        assert len(names) >= 400 and {b"@s0", b"@s50"} <= set(names)
        assert b"of 20000 reads." in d.stderr


def test_reuse_across_inputs(dcli, tmp_path):
    """Two different inputs through one process, one filter, in both orders: each result is independent of the other."""
    a, b = F.reads_text(51, 400), bgzf(F.reads_text(52, 300, lo=300, hi=2000), 4000)
    outs = {}
    for order in ("ab", "ba", "b"):
        d = tmp_path / order
        d.mkdir()
        paths = []
        for k in order:
            p = d / (k + ".fq")
            p.write_bytes(a if k == "a" else b)
            paths.append(p)
        lst = d / "list.txt"
        lst.write_text("".join(str(p) + "\n" for p in paths))
        r = subprocess.run([dcli, "--fastq-subset-each", str(lst), "--device", "-l", "42", "--fastq-chunk-bytes", "50000"],
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-300:]
        for p in paths:
            assert (d / (p.name + ".ok")).exists(), (d / (p.name + ".err")).read_text() if (d / (p.name + ".err")).exists() else p
        outs[order] = {p.name: (d / (p.name + ".out")).read_bytes() for p in paths}
    assert outs["ab"]["b.fq"] == outs["ba"]["b.fq"] == outs["b"]["b.fq"]
    assert outs["ab"]["a.fq"] == outs["ba"]["a.fq"]
    rf = OracleReadFilter(H.parse_cli("--fastq-subset -l 42"))
    assert outs["ab"]["a.fq"] == F.ref_subset(a, rf)[0] and len(outs["b"]["b.fq"]) > 1000


@pytest.mark.parametrize("mix", ["eof_between", "no_eof", "trailing", "trailing_no_eof"])
def test_bgzf_members_then_plain_gzip(dcli, tmp_path, mix):
    """BGZF members followed by a plain gzip member, cut in the middle of a record: the device route inflates the members on the
    GPU and hands the rest of the file to zlib; zlib reads the whole file as concatenated gzip members.  With and without the
    BGZF EOF marker in between, with chunks small enough that the foreign member is the first of a fill and large enough that
    it is met in the middle of one.  Bytes that are not gzip behind the members end the input, as zlib ignores them."""
    text = F.reads_text(71, 120, lo=30, hi=400)
    want, kept, total = F.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset -l 42")))
    assert 0 < kept < total == 120
    cut = len(text) // 2 + 7
    members, whole = bgzf(text[:cut], 600), bgzf(text, 600)
    data = {"eof_between": members + gzip.compress(text[cut:], 6), "no_eof": members[:-len(EOF_BLOCK)] + gzip.compress(text[cut:], 6),
            "trailing": whole + b"not gzip at all\n", "trailing_no_eof": whole[:-len(EOF_BLOCK)] + b"xy"}[mix]
    p = tmp_path / (mix + ".fq.gz")
    p.write_bytes(data)
    for chunk in (["--fastq-chunk-bytes", "1000", "--reads-per-batch", "5"], ["--fastq-chunk-bytes", "4096"], []):
        d, _ = both(dcli, ["-l", "42"] + chunk, path=p, timeout=120)
        assert d.returncode == 0 and d.stdout == want, (mix, chunk, d.stderr[-300:])
        assert ("FASTQ subset: kept %d of %d reads." % (kept, total)).encode() in d.stderr


def test_record_larger_than_the_compressed_buffer(dcli, tmp_path):
    """A 300 kb read through 1 000-byte chunks of a bgzipped file: the chunk doubles per refill although one inflate call
    takes about a chunk of compressed bytes (several calls fill it)."""
    rng = np.random.default_rng(9)
    big = seqgen.random_dna(rng, 300_000).tobytes()[:-600] + b"TTAGGG" * 100
    text = F.reads_text(72, 20) + F.record_text(b"big", big) + F.reads_text(73, 20)
    want, kept, total = F.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset -l 42")))
    assert b"@big\n" in want and total == 41
    p = tmp_path / "bigz.fq.gz"
    p.write_bytes(bgzf_fancy(text, 65000, random.Random(2)))
    d, _ = both(dcli, ["-l", "42", "--fastq-chunk-bytes", "1000"], path=p, timeout=120)
    assert d.returncode == 0 and d.stdout == want, d.stderr[-300:]


def test_damaged_bgzf_is_an_error_not_a_signal(dcli, tmp_path):
    """A flipped payload bit and a wrong CRC in a bgzipped input: the device run exits 1 with Error: on stderr.  (The host
    route's verdict is not required here: zlib's streaming reader treats damaged, truncated and trailing data its own way.)"""
    text = F.reads_text(61, 300)
    good = bytearray(bgzf(text, 3000))
    flipped = bytearray(good)
    flipped[18 + 40] ^= 0x10                                        # inside the first member's deflate payload
    first_total = int.from_bytes(good[16:18], "little") + 1
    crc = bytearray(good)
    crc[first_total - 8] ^= 0xff                                    # the first member's CRC32
    for name, data in (("flipped", flipped), ("crc", crc)):
        p = tmp_path / (name + ".fq.gz")
        p.write_bytes(bytes(data))
        r = subprocess.run([dcli, "--fastq-subset", "--device", "-l", "42", str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stderr.startswith(b"Error:"), (name, r.returncode, r.stderr[-200:])
