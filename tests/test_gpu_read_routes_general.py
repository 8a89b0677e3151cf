"""The two read device routes on pattern sets the tiled kernel does not take (mixed lengths, 9 bases and more, the wide form):
fastqSubsetDevice and bamSubsetDevice through the two test CLIs, --device against --host of the same binary on the same input —
return code 0, byte-equal stdout, the same `kept K of T` line — and against the CPU oracle's read filter.  The batch calls
behind the routes are tested one by one in tests/test_gpu_read_batch_general.py."""
import os
import re
import subprocess

import pytest

from tests import readsets as R
from tests.test_bam_subset import bgzf, build_bam
from tests.test_fastq_chunk_reference_cpu import build_cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--fastq-chunk-bytes", "1000", "--reads-per-batch", "3"]


@pytest.fixture(scope="module")
def fq_cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "fastq_device_cli")


@pytest.fixture(scope="module")
def bam_cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401
    out = tmp_path_factory.mktemp("cpp") / "bam_device_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bam_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def both(cli, mode, args, path, timeout=120):
    """The device run and the host run of the same command: rc 0 both, byte-equal stdout, the same last line of stderr
    (`... kept K of T ...`); -> (the device run, K, T)."""
    res = []
    for route in ("--device", "--host"):
        res.append(subprocess.run([cli, mode, route] + list(args) + [str(path)], stdin=subprocess.DEVNULL, capture_output=True,
                                  timeout=timeout))
    d, h = res
    assert d.returncode == 0 and h.returncode == 0, (d.returncode, h.returncode, d.stderr[-400:], h.stderr[-400:])
    assert d.stdout == h.stdout
    kept = [re.search(rb"kept (\d+) of (\d+) ", r.stderr) for r in res]
    assert kept[0] and kept[1] and kept[0].groups() == kept[1].groups(), (d.stderr[-300:], h.stderr[-300:])
    return d, int(kept[0].group(1)), int(kept[0].group(2))


def kept_fastq(reads, passes):
    return b"".join(rec for rec, p in zip(R.fastq_records(reads), passes) if p)


@pytest.mark.parametrize("flags", R.SETS, ids=R.SET_IDS)
def test_fastq_route_on_general_sets(fq_cli, tmp_path, flags):
    """Without general tips batches --device exits 1 here: "cannot plan the read batch: unsupported parameter set"."""
    reads = R.reads_for(flags)
    passes = R.oracle_passes(flags)
    text = R.fastq_text(reads)
    files = {"plain": tmp_path / "in.fq", "bgzf": tmp_path / "in.fq.gz"}
    files["plain"].write_bytes(text)
    files["bgzf"].write_bytes(bgzf(text, 3000))
    for kind in ("plain", "bgzf"):
        for chunk in ([], SMALL):
            d, k, t = both(fq_cli, "--fastq-subset", flags.split() + chunk, files[kind])
            assert t == len(reads) and 0 < k < t and k == sum(passes), (kind, chunk)
            assert d.stdout == kept_fastq(reads, passes), (kind, chunk)


def test_fastq_route_crlf(fq_cli, tmp_path):
    flags = R.SETS[0]
    reads, passes = R.reads_for(flags), R.oracle_passes(flags)
    p = tmp_path / "crlf.fq"
    p.write_bytes(R.fastq_text(reads, b"\r\n"))
    for chunk in ([], SMALL):
        d, k, t = both(fq_cli, "--fastq-subset", flags.split() + chunk, p)
        assert (k, t) == (sum(passes), len(reads)) and 0 < k < t


@pytest.mark.parametrize("flags", [R.SETS[0], R.SETS[2], R.SETS[3]], ids=[R.SET_IDS[0], R.SET_IDS[2], R.SET_IDS[3]])
def test_bam_route_on_general_sets(bam_cli, tmp_path, flags):
    reads, passes = R.reads_for(flags), R.oracle_passes(flags)
    named = [("r%d" % i, r.decode()) for i, r in enumerate(reads)]
    _, _, bam = build_bam(named, 20000)                             # BGZF members of 20 000 bytes
    p = tmp_path / "in.bam"
    p.write_bytes(bam)
    for chunk in ([], ["--bam-chunk-bytes", str(1 << 20), "--reads-per-batch", "5"]):   # (the route's smallest chunk; many batches)
        d, k, t = both(bam_cli, "--bam-subset", flags.split() + chunk, p)
        assert t == len(reads) and k == sum(passes) and 0 < k < t, chunk
        assert len(d.stdout) > 28                                   # more than the EOF member


def test_overflow_through_the_fastq_route(fq_cli, tmp_path):
    """The dense set whose tiles overflow their slots: the route's regrow-and-rescan (ReadJudge's protocol) gives the host's bytes."""
    reads = R.overflow_reads()
    p = tmp_path / "dense.fq"
    p.write_bytes(R.fastq_text(reads))
    for chunk in ([], ["--fastq-chunk-bytes", "40000", "--reads-per-batch", "2"]):
        d, k, t = both(fq_cli, "--fastq-subset", R.OVERFLOW_SET.split() + chunk, p)
        assert t == len(reads) and 0 < k < t


def test_a_tiled_set_is_untouched(fq_cli, tmp_path):
    flags = "-x 0 -l 18 -y 0.8 -k 10 -d 10"
    reads = R.reads_for(flags)
    from tests.backends import OracleReadFilter
    passes = OracleReadFilter(R.options(flags)).filter(reads)
    p = tmp_path / "tiled.fq"
    p.write_bytes(R.fastq_text(reads))
    for chunk in ([], SMALL):
        d, k, t = both(fq_cli, "--fastq-subset", flags.split() + chunk, p)
        assert (k, t) == (sum(passes), len(reads)) and 0 < k < t
        assert d.stdout == kept_fastq(reads, passes)
