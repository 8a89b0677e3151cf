"""bamSubsetDevice with BamOutputDeflate::Device through tests/cpp/bam_deflate_cli.cpp, on the scenarios of
tests/test_gpu_bam_device.py, every one of them.  --deflate host writes exactly the bytes bam_device_cli --device writes; --deflate device writes a
BGZF file of valid members that ends in the EOF marker, begins with the host-compressed header members, inflates to what the
host form's output inflates to, and is the same file on one, two and three contexts.  Errors are the host form's errors; the
library's counters show that every passing record byte went through ts_bam_chunk_gather_bgzf under device and none under host."""
import os
import random
import re
import subprocess
import zlib

import numpy as np
import pytest

from tests import seqgen
from tests.test_bam_subset import EOF_BLOCK, _kept_names, bgzf, bgzf_fancy, build_bam, make_reads
from tests.test_gpu_bam_device import dcli, mutation_files_70  # noqa: F401  (dcli: the fixture that builds bam_device_cli)
from tests.test_gpu_bgzf_deflate import members_of
from tests.test_inflate_core_cpu import mutation_files_512

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = re.compile(rb"deflate: calls (\d+) members (\d+) plain (\d+) out (\d+); route: plain (\d+) out (\d+)")


@pytest.fixture(scope="module")
def zcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / "bam_deflate_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bam_deflate_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def run(exe, args, path=None, stdin_path=None, timeout=300):
    cmd = [exe, "--bam-subset"] + args + ([str(path)] if path is not None else [])
    return subprocess.run(cmd, stdin=open(stdin_path, "rb") if stdin_path else subprocess.DEVNULL, capture_output=True, timeout=timeout)


def counters(r):
    m = COUNTERS.search(r.stderr)
    assert m, r.stderr[-500:]
    return [int(x) for x in m.groups()]


def inflate_file(data):
    """A BGZF file -> (its members' plain bytes joined, [member's plain size]); every member valid, the EOF marker last."""
    assert data.endswith(EOF_BLOCK)
    plain, sizes = b"", []
    for payload, crc, isize in members_of(data[:-len(EOF_BLOCK)]):
        d = zlib.decompressobj(-15)
        piece = d.decompress(payload)
        assert d.eof and not d.unused_data and len(piece) == isize and zlib.crc32(piece) & 0xFFFFFFFF == crc
        plain += piece
        sizes.append(isize)
    return plain, sizes


def compare(zcli, dcli, args, path=None, stdin_path=None, contexts=("0,0",), header=None):  # noqa: F811
    """One input through bam_device_cli --device, --deflate host and --deflate device on 1 context and on `contexts`.  -> the
    device form's result."""
    old = run(dcli, ["--device"] + args, path, stdin_path)
    host = run(zcli, ["--deflate", "host"] + args, path, stdin_path)
    dev = run(zcli, ["--deflate", "device"] + args, path, stdin_path)
    assert old.returncode == host.returncode == dev.returncode, (old.stderr[-300:], host.stderr[-300:], dev.stderr[-300:])
    assert host.stdout == old.stdout                               # the default path did not move
    if old.returncode != 0:
        def message(r):
            return [line for line in r.stderr.splitlines() if line.startswith(b"Error:")]
        assert message(old) == message(host) == message(dev) and message(old)
        return dev
    assert counters(host) == [0, 0, 0, 0, 0, 0]                    # under host the new counters do not move
    want, _ = inflate_file(host.stdout)
    got, sizes = inflate_file(dev.stdout)
    assert got == want
    calls, members, plain_in, out, route_plain, route_out = counters(dev)
    if header is not None:
        assert want[:len(header)] == header
        passing = len(want) - len(header)
        assert plain_in == route_plain == passing                  # every passing record byte went through the device encoder
        assert out == route_out and (calls > 0) == (passing > 0)
        # the header's members come first, compressed on the host into members of their own (where no read passes the file is
        # the host form's, byte for byte: test_every_read_passes_and_none_passes); the device's members follow, then the marker
        head_members = -(-len(header) // 0xFF00)
        assert sum(sizes[:head_members]) == len(header)
        at = 0
        for _ in range(head_members):
            at += int.from_bytes(dev.stdout[at + 16:at + 18], "little") + 1
        assert len(dev.stdout) == at + out + len(EOF_BLOCK)
    for ctxs in contexts:
        multi = run(zcli, ["--deflate", "device", "--devices", ctxs] + args, path, stdin_path)
        assert multi.returncode == 0, multi.stderr[-300:]
        assert multi.stdout == dev.stdout, ctxs                    # the same file whatever the number of contexts
        assert counters(multi)[2:] == counters(dev)[2:], ctxs
    return dev


@pytest.mark.parametrize("flags,chunk,via_stdin", [("", 60000, False), ("-l 42", 1000, False), ("-x 0 -l 18 -y 0.8 -k 10 -d 10", 64000, True)])
def test_device_deflate_matches_host_deflate(zcli, dcli, tmp_path, flags, chunk, via_stdin):  # noqa: F811
    header, records, bam = build_bam(make_reads(), chunk)
    path = tmp_path / "in.bam"
    path.write_bytes(bam)
    r = compare(zcli, dcli, flags.split(), path=None if via_stdin else path, stdin_path=path if via_stdin else None, header=header)
    assert r.returncode == 0 and b"BAM subset: kept" in r.stderr


def test_chunks_sub_batches_and_large_records(zcli, dcli, tmp_path):  # noqa: F811
    gen = random.Random(5)
    rng = np.random.default_rng(123)
    reads = make_reads()
    big = bytearray(seqgen.random_dna(rng, 1_400_000).tobytes())
    t = seqgen.repeat_array("CCCTAA", 2000).tobytes()
    big[-len(t):] = t
    reads.insert(200, ("big_telomeric", big.decode()))
    reads.insert(300, ("big_plain", seqgen.random_dna(rng, 1_200_000).tobytes().decode()))
    header, records, _ = build_bam(reads, 60000)
    path = tmp_path / "fancy.bam"
    path.write_bytes(bgzf_fancy(header + b"".join(records), 30011, gen))
    r = compare(zcli, dcli, ["--bam-chunk-bytes", str(1 << 20), "--reads-per-batch", "97"], path=path, header=header,
                contexts=("0,0", "0,0,0"))
    assert r.returncode == 0 and counters(r)[1] > 10               # the large record alone is eleven members


def test_every_read_passes_and_none_passes(zcli, dcli, tmp_path):  # noqa: F811
    rng = np.random.default_rng(9)
    telomeric = [("t%d" % i, ("TTAGGG" * 400)[:int(rng.integers(600, 2400))]) for i in range(600)]
    plain = [("p%d" % i, seqgen.random_dna(rng, int(rng.integers(100, 900))).tobytes().decode()) for i in range(600)]
    for name, reads, all_pass in (("all", telomeric, True), ("none", plain, False)):
        header, records, bam = build_bam(reads, 60000)
        path = tmp_path / (name + ".bam")
        path.write_bytes(bam)
        r = compare(zcli, dcli, ["--bam-chunk-bytes", str(1 << 20), "--reads-per-batch", "250"], path=path, header=header,
                    contexts=("0,0", "0,0,0"))
        got, _ = inflate_file(r.stdout)
        if all_pass:
            assert got == header + b"".join(records) and counters(r)[0] >= 3
        else:
            assert got == header and counters(r) == [0, 0, 0, 0, 0, 0]      # header and EOF marker only
            host = run(zcli, ["--deflate", "host", "--bam-chunk-bytes", str(1 << 20)], path)
            assert r.stdout == host.stdout


def test_errors_are_the_host_forms(zcli, dcli, tmp_path):  # noqa: F811
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bgzf(b"NOTBAM" + b"\0" * 100, 60000))
    r = compare(zcli, dcli, [], path=bad)
    assert r.returncode != 0 and b"not a BAM" in r.stderr
    header, records, bam = build_bam(make_reads()[:8], 60000)
    noeof = tmp_path / "noeof.bam"
    noeof.write_bytes(bam[:-len(EOF_BLOCK)])
    r = compare(zcli, dcli, [], path=noeof, header=header)
    assert r.returncode == 0 and b"missing the BGZF EOF marker" in r.stderr
    # damaged members of an otherwise valid file of many members: flags bit, BC length, wrong magic
    reads = make_reads()
    header, records, _ = build_bam(reads, 60000)
    good = bgzf_fancy(header + b"".join(records), 30011, random.Random(5))
    for what, damage in (("flags", lambda b: b[:3] + bytes([b[3] | 0x20]) + b[4:]),
                         ("bc length", lambda b: b[:14] + b"\x03" + b[15:]),
                         ("not gzip", lambda b: b"\x1f\x8c" + b[2:])):
        bad.write_bytes(damage(good))
        r = compare(zcli, dcli, [], path=bad)
        assert r.returncode == 1 and b"Error:" in r.stderr, (what, r.returncode, r.stderr[-200:])


def each_form(zcli, tmp_path, files, timeout):
    """Every file through ONE --deflate host process and ONE --deflate device process (--bam-subset-each): per file the same
    verdict, the same counts or the same message, and outputs that inflate to the same bytes.  -> (ok files, refused files)"""
    verdicts = {}
    for form in ("host", "device"):
        d = tmp_path / form
        d.mkdir()
        paths = []
        for i, data in enumerate(files):
            p = d / ("m%03d.bam" % i)
            p.write_bytes(data)
            paths.append(p)
        lst = d / "list.txt"
        lst.write_text("".join(str(p) + "\n" for p in paths))
        r = subprocess.run([zcli, "--bam-subset-each", str(lst), "--deflate", form, "-x", "0", "-l", "18"], capture_output=True, timeout=timeout)
        assert r.returncode == 0, (form, r.stderr[-500:])
        out = []
        for p in paths:
            ok, err, res = (p.parent / (p.name + ext) for ext in (".ok", ".err", ".out"))
            assert ok.exists() != err.exists(), (form, p.name)
            out.append(("ok", ok.read_text(), res.read_bytes()) if ok.exists() else ("err", err.read_text(), None))
        verdicts[form] = out
    n_ok = 0
    for i, (dv, hv) in enumerate(zip(verdicts["device"], verdicts["host"])):
        assert dv[:2] == hv[:2], (i, dv[:2], hv[:2])              # the same verdict, counts or message
        if dv[0] == "ok":
            assert inflate_file(dv[2])[0] == inflate_file(hv[2])[0], i
            n_ok += 1
        else:
            assert dv[1].strip(), i
    return n_ok, len(files) - n_ok


def test_mutation_suite_70(zcli, tmp_path):
    n_ok, n_err = each_form(zcli, tmp_path, mutation_files_70(), 300)
    assert n_ok >= 5 and n_err >= 20, (n_ok, n_err)


def test_mutation_suite_512(zcli, tmp_path):
    n_ok, n_err = each_form(zcli, tmp_path, mutation_files_512(), 600)
    assert n_ok >= 40 and n_err >= 150, (n_ok, n_err)


def kept_names(zcli, dcli, tmp_path, reads, flags, tag):  # noqa: F811
    header, records, bam = build_bam(reads, 60000)
    path = tmp_path / ("%s.bam" % tag)
    path.write_bytes(bam)
    r = compare(zcli, dcli, flags, path=path, header=header, contexts=())
    assert r.returncode == 0, r.stderr
    return _kept_names(inflate_file(r.stdout)[0], header)


def test_threshold_known_answers(zcli, dcli, tmp_path):  # noqa: F811
    default = [("short", "TTAGGG" * 6), ("default_pass", "TTAGGG" * 7), ("long", "CCCTAA" * 15), ("fail", "ACGT" * 20)]
    assert kept_names(zcli, dcli, tmp_path, default, [], "d") == ["default_pass", "long"]
    lengths = [("one_repeat", "TTAGGG"), ("exact_12", "TTAGGG" * 2), ("flanked_exact", "ACGT" + "CCCTAA" * 2 + "TGCA"),
               ("exact_18", "TTAGGG" * 3)]
    l12 = ["-x", "0", "-l", "12", "-y", "1", "-k", "10", "-d", "10"]
    l18 = ["-x", "0", "-l", "18", "-y", "1", "-k", "10", "-d", "10"]
    assert kept_names(zcli, dcli, tmp_path, lengths, l12, "l12") == ["exact_12", "flanked_exact", "exact_18"]
    assert kept_names(zcli, dcli, tmp_path, lengths, l18, "l18") == ["exact_18"]
    density = [("two_thirds", "TTAGGGAAAAAATTAGGG")]
    assert kept_names(zcli, dcli, tmp_path, density, ["-x", "0", "-l", "18", "-y", "0.666", "-k", "20", "-d", "10"], "y1") == ["two_thirds"]
    assert kept_names(zcli, dcli, tmp_path, density, ["-x", "0", "-l", "18", "-y", "0.667", "-k", "20", "-d", "10"], "y2") == []
    plant = [("plant_pass", "TTTAGGG" * 3), ("vertebrate_fail", "TTAGGG" * 4)]
    assert kept_names(zcli, dcli, tmp_path, plant, ["-c", "CCCTAAA", "-x", "0", "-l", "21", "-y", "1"], "p") == ["plant_pass"]


def test_short_reads(zcli, dcli, tmp_path):  # noqa: F811
    """20 000 reads of 100-300 bases, some 400 of them passing: many small records through gather and deflate."""
    rng = np.random.default_rng(31)
    reads = []
    for i in range(20000):
        n = int(rng.integers(100, 301))
        s = seqgen.random_dna(rng, n).tobytes().decode()
        if i % 50 == 0:
            s = ("TTAGGG" * 60)[:n]
        reads.append(("s%d" % i, s))
    header, records, bam = build_bam(reads, 60000)
    path = tmp_path / "short.bam"
    path.write_bytes(bam)
    r = compare(zcli, dcli, ["-l", "42", "--bam-chunk-bytes", str(1 << 20), "--reads-per-batch", "3000"], path=path, header=header)
    assert r.returncode == 0, r.stderr[-300:]
    names = _kept_names(inflate_file(r.stdout)[0], header)
    assert len(names) >= 400 and {"s0", "s50"} <= set(names)
    assert counters(r)[0] >= 3                                      # several sub-batches, each deflated on its own


def test_reuse_across_inputs(zcli, tmp_path):
    """Two different BAMs through one process, one filter, one chunk and its deflate buffers: the second result does not depend
    on the first, under device as under host."""
    reads = make_reads()
    _, _, bam_a = build_bam(reads[:200], 60000)
    _, _, bam_b = build_bam(reads[150:], 3000)
    outs = {}
    for form in ("device", "host"):
        for order in ("ab", "ba", "b"):
            d = tmp_path / (form + "_" + order)
            d.mkdir()
            paths = []
            for k in order:
                p = d / (k + ".bam")
                p.write_bytes(bam_a if k == "a" else bam_b)
                paths.append(p)
            lst = d / "list.txt"
            lst.write_text("".join(str(p) + "\n" for p in paths))
            r = subprocess.run([zcli, "--bam-subset-each", str(lst), "--deflate", form, "-l", "42"], capture_output=True, timeout=300)
            assert r.returncode == 0, r.stderr[-300:]
            outs[form, order] = {p.name: (d / (p.name + ".out")).read_bytes() for p in paths}
    dev = {order: outs["device", order] for order in ("ab", "ba", "b")}
    assert dev["ab"]["b.bam"] == dev["ba"]["b.bam"] == dev["b"]["b.bam"]
    assert dev["ab"]["a.bam"] == dev["ba"]["a.bam"]
    for name in ("a.bam", "b.bam"):
        assert inflate_file(dev["ab"][name])[0] == inflate_file(outs["host", "ab"][name])[0], name
    assert len(inflate_file(dev["b"]["b.bam"])[0]) > 1000
