"""The device route of --bam-subset (bamSubsetDevice: BGZF members inflated, records walked, SEQ decoded and passing records
gathered on the GPU) through tests/cpp/bam_device_cli.cpp: every scenario of tests/test_bam_subset.py with --device, asserting
what those tests assert and that stdout is byte-equal to the --host run of the same binary on the same file.  The stages
behind the inflate (record walk, SEQ decode, carry, gather) are compared one by one with plain references in
tests/test_gpu_bam_chunk.py."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import harness as H
from tests import seqgen
from tests.backends import OracleReadFilter
from tests.test_bam_subset import EOF_BLOCK, _kept_names, bgzf, bgzf_fancy, build_bam, gunzip_members, make_reads
from tests.test_inflate_core_cpu import mutation_files_512

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / "bam_device_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bam_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def both(dcli, args, path=None, stdin_path=None, timeout=600):
    """The device run and the host run of the same command: (device result, host result); stdout equal when both succeed."""
    res = []
    for route in ("--device", "--host"):
        cmd = [dcli, "--bam-subset", route] + args + ([str(path)] if path is not None else [])
        res.append(subprocess.run(cmd, stdin=open(stdin_path, "rb") if stdin_path else subprocess.DEVNULL,
                                  capture_output=True, timeout=timeout))
    d, h = res
    assert d.returncode == h.returncode, (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.stdout == h.stdout
    return d, h


@pytest.mark.parametrize("flags,chunk,via_stdin", [("", 60000, False), ("-l 42", 1000, False), ("-x 0 -l 18 -y 0.8 -k 10 -d 10", 64000, True)])
def test_device_route_matches_oracle_and_host(dcli, tmp_path, flags, chunk, via_stdin):
    reads = make_reads()
    header, records, bam = build_bam(reads, chunk)
    path = tmp_path / "in.bam"
    path.write_bytes(bam)
    r, _ = both(dcli, flags.split(), path=None if via_stdin else path, stdin_path=path if via_stdin else None)
    assert r.returncode == 0, r.stderr
    opts = H.parse_cli("--fastq-subset " + flags)
    with_seq = [i for i, (_, s) in enumerate(reads) if s]
    passes = OracleReadFilter(opts).filter([reads[i][1].encode() for i in with_seq])
    keep = [i for i, ok in zip(with_seq, passes) if ok]
    assert 0 < len(keep) < len(with_seq)
    out = r.stdout
    assert out.endswith(EOF_BLOCK) and out[:4] == b"\x1f\x8b\x08\x04"
    plain = gunzip_members(out)
    assert plain[:len(header)] == header
    assert plain[len(header):] == b"".join(records[i] for i in keep)
    err = r.stderr.decode()
    assert "BAM subset: kept %d of %d records." % (len(keep), len(reads)) in err
    assert "BAM subset: skipped 1 record without SEQ." in err


def test_device_route_rejects_garbage_and_flags_missing_eof(dcli, tmp_path):
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bgzf(b"NOTBAM" + b"\0" * 100, 60000))
    r, h = both(dcli, [], path=bad, timeout=120)
    assert r.returncode != 0 and b"not a BAM" in r.stderr and b"not a BAM" in h.stderr
    header, records, bam = build_bam(make_reads()[:8], 60000)
    noeof = tmp_path / "noeof.bam"
    noeof.write_bytes(bam[:-len(EOF_BLOCK)])
    r, _ = both(dcli, [], path=noeof, timeout=120)
    assert r.returncode == 0 and b"missing the BGZF EOF marker" in r.stderr


def _run(dcli, tmp_path, reads, flags, tag):
    header, records, bam = build_bam(reads, 60000)
    path = tmp_path / ("%s.bam" % tag)
    path.write_bytes(bam)
    r, _ = both(dcli, flags, path=path, timeout=120)
    assert r.returncode == 0, r.stderr
    return _kept_names(gunzip_members(r.stdout), header)


def test_device_route_threshold_known_answers(dcli, tmp_path):
    default = [("short", "TTAGGG" * 6), ("default_pass", "TTAGGG" * 7), ("long", "CCCTAA" * 15), ("fail", "ACGT" * 20)]
    assert _run(dcli, tmp_path, default, [], "d") == ["default_pass", "long"]
    lengths = [("one_repeat", "TTAGGG"), ("exact_12", "TTAGGG" * 2), ("flanked_exact", "ACGT" + "CCCTAA" * 2 + "TGCA"),
               ("exact_18", "TTAGGG" * 3)]
    l12 = ["-x", "0", "-l", "12", "-y", "1", "-k", "10", "-d", "10"]
    l18 = ["-x", "0", "-l", "18", "-y", "1", "-k", "10", "-d", "10"]
    assert _run(dcli, tmp_path, lengths, l12, "l12") == ["exact_12", "flanked_exact", "exact_18"]
    assert _run(dcli, tmp_path, lengths, l18, "l18") == ["exact_18"]
    density = [("two_thirds", "TTAGGGAAAAAATTAGGG")]
    assert _run(dcli, tmp_path, density, ["-x", "0", "-l", "18", "-y", "0.666", "-k", "20", "-d", "10"], "y1") == ["two_thirds"]
    assert _run(dcli, tmp_path, density, ["-x", "0", "-l", "18", "-y", "0.667", "-k", "20", "-d", "10"], "y2") == []
    plant = [("plant_pass", "TTTAGGG" * 3), ("vertebrate_fail", "TTAGGG" * 4)]
    assert _run(dcli, tmp_path, plant, ["-c", "CCCTAAA", "-x", "0", "-l", "21", "-y", "1"], "p") == ["plant_pass"]


def test_device_route_blocks_chunks_and_large_records(dcli, tmp_path):
    gen = random.Random(5)
    rng = np.random.default_rng(123)
    reads = make_reads()
    big = bytearray(seqgen.random_dna(rng, 1_400_000).tobytes())
    t = seqgen.repeat_array("CCCTAA", 2000).tobytes()
    big[-len(t):] = t
    reads.insert(200, ("big_telomeric", big.decode()))
    reads.insert(300, ("big_plain", seqgen.random_dna(rng, 1_200_000).tobytes().decode()))
    header, records, _ = build_bam(reads, 60000)
    payload = header + b"".join(records)
    path = tmp_path / "fancy.bam"
    path.write_bytes(bgzf_fancy(payload, 30011, gen))
    r, _ = both(dcli, ["--bam-chunk-bytes", str(1 << 20), "--reads-per-batch", "97"], path=path)
    assert r.returncode == 0, r.stderr[-500:]
    opts = H.parse_cli("--fastq-subset")
    with_seq = [i for i, (_, s) in enumerate(reads) if s]
    passes = OracleReadFilter(opts).filter([reads[i][1].encode() for i in with_seq])
    keep = [i for i, ok in zip(with_seq, passes) if ok]
    assert reads.index(("big_telomeric", big.decode())) in keep
    plain = gunzip_members(r.stdout)
    assert plain[:len(header)] == header
    assert plain[len(header):] == b"".join(records[i] for i in keep)
    assert b"missing the BGZF EOF marker" not in r.stderr
    r2, _ = both(dcli, ["--bam-chunk-bytes", str(1 << 20)], stdin_path=path)
    assert r2.returncode == 0 and gunzip_members(r2.stdout) == plain
    good = bgzf_fancy(payload, 30011, random.Random(5))
    for what, damage in (("flags", lambda b: b[:3] + bytes([b[3] | 0x20]) + b[4:]),
                         ("bc length", lambda b: b[:14] + b"\x03" + b[15:]),
                         ("not gzip", lambda b: b"\x1f\x8c" + b[2:])):
        bad = tmp_path / "bad.bam"
        bad.write_bytes(damage(good))
        r3, _ = both(dcli, [], path=bad, timeout=120)
        assert r3.returncode == 1 and b"Error:" in r3.stderr, (what, r3.returncode, r3.stderr[-200:])


def mutation_files_70():
    """The 70 files of tests/test_bam_subset.py::test_bam_mutation_robustness, from the same seed."""
    gen = random.Random(91)
    reads = [("record_%d" % i, "TTAGGG" * (3 + i % 5)) for i in range(8)]
    header, records, _ = build_bam(reads, 60000)
    payload = header + b"".join(records)
    roff = len(header)
    files = []
    for index in range(70):
        mode = index % 7
        if mode == 0:
            data = bytes(gen.getrandbits(8) for _ in range(gen.randrange(0, 2048)))
        elif mode == 1:
            data = bgzf(payload[:gen.randrange(len(payload) + 1)], 60000)
        elif mode == 2:
            m = bytearray(payload)
            m[gen.randrange(roff + 36, len(m))] ^= 1 << gen.randrange(8)
            data = bgzf(bytes(m), 60000)
        elif mode == 3:
            m = bytearray(payload)
            struct.pack_into("<i", m, roff, gen.randrange(-16, 129))
            data = bgzf(bytes(m), 60000)
        elif mode == 4:
            m = bytearray(payload)
            m[roff + 12] = gen.randrange(256)
            data = bgzf(bytes(m), 60000)
        elif mode == 5:
            m = bytearray(payload)
            struct.pack_into("<H", m, roff + 16, gen.randrange(65536))
            data = bgzf(bytes(m), 60000)
        else:
            data = bgzf(header + b"".join(records[:gen.randrange(len(records) + 1)]), 60000)
        files.append(data)
    return files


def each(dcli, tmp_path, files, timeout):
    """Every file through ONE device process and ONE host process (--bam-subset-each): per file the same verdict, equal
    bytes when ok, the same message when not.  A fault of the device ends its process, and with it the suite."""
    verdicts = {}
    for route in ("device", "host"):
        d = tmp_path / route
        d.mkdir()
        paths = []
        for i, data in enumerate(files):
            p = d / ("m%03d.bam" % i)
            p.write_bytes(data)
            paths.append(p)
        lst = d / "list.txt"
        lst.write_text("".join(str(p) + "\n" for p in paths))
        r = subprocess.run([dcli, "--bam-subset-each", str(lst), "--" + route, "-x", "0", "-l", "18"], capture_output=True, timeout=timeout)
        assert r.returncode == 0, (route, r.returncode, r.stderr[-500:])
        out = []
        for p in paths:
            ok, err, res = (p.parent / (p.name + ext) for ext in (".ok", ".err", ".out"))
            assert ok.exists() != err.exists(), (route, p.name)
            out.append(("ok", ok.read_text(), res.read_bytes()) if ok.exists() else ("err", err.read_text(), None))
        verdicts[route] = out
    n_ok = 0
    for i, (dv, hv) in enumerate(zip(verdicts["device"], verdicts["host"])):
        assert dv[0] == hv[0], (i, dv[:2], hv[:2])
        assert dv[2] == hv[2], i
        if dv[0] == "ok":
            assert dv[1] == hv[1], i
            assert dv[2].endswith(EOF_BLOCK), i
            n_ok += 1
        else:
            assert dv[1].strip(), i
    return n_ok, len(files) - n_ok


def test_device_route_mutation_suite_70(dcli, tmp_path):
    n_ok, n_err = each(dcli, tmp_path, mutation_files_70(), 300)
    assert n_ok >= 5 and n_err >= 20, (n_ok, n_err)


def test_device_route_mutation_suite_512(dcli, tmp_path):
    n_ok, n_err = each(dcli, tmp_path, mutation_files_512(), 600)
    assert n_ok >= 40 and n_err >= 150, (n_ok, n_err)


def test_device_route_short_reads(dcli, tmp_path):
    """20 000 reads of 100-300 bases: the walk's many-records case."""
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
    r, _ = both(dcli, ["-l", "42"], path=path)
    assert r.returncode == 0, r.stderr[-300:]
    names = _kept_names(gunzip_members(r.stdout), header)
    assert len(names) >= 400 and {"s0", "s50"} <= set(names)


def test_device_route_reuse_across_inputs(dcli, tmp_path):
    """Two different BAMs through one process, one filter: the second result does not depend on the first."""
    reads = make_reads()
    _, _, bam_a = build_bam(reads[:200], 60000)
    _, _, bam_b = build_bam(reads[150:], 3000)
    outs = {}
    for order in ("ab", "ba", "b"):
        d = tmp_path / order
        d.mkdir()
        paths = []
        for k in order:
            p = d / (k + ".bam")
            p.write_bytes(bam_a if k == "a" else bam_b)
            paths.append(p)
        lst = d / "list.txt"
        lst.write_text("".join(str(p) + "\n" for p in paths))
        r = subprocess.run([dcli, "--bam-subset-each", str(lst), "--device", "-l", "42"], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-300:]
        outs[order] = {p.name: (d / (p.name + ".out")).read_bytes() for p in paths}
    assert outs["ab"]["b.bam"] == outs["ba"]["b.bam"] == outs["b"]["b.bam"]
    assert outs["ab"]["a.bam"] == outs["ba"]["a.bam"]
    assert len(gunzip_members(outs["b"]["b.bam"])) > 1000
