"""fastqSubsetDevice and bamSubsetDevice on a ReadTelomereFilter of several contexts (the input's chunks dealt to all of them:
include/teloscope_mi355x_ring.hpp and the routes' chunk steps of include/teloscope_mi355x_io.hpp) through
tests/cpp/read_routes_multi_cli.cpp: 2 and 3 contexts on this one GPU against 1 context and against the host route of the same
binary — equal verdicts, byte-equal output, equal result structs, equal messages and equal bytes written before a failure — and
the per-context figures, which say that every context worked.  One set of steps serves every count (one context fills each chunk
in place, on the caller's thread and with no staging region; on several the ring deals the chunks), so 1 against N contexts
compares two ways in of one code: the independent side is the host route, and the figures of one context are held against the
chunks the parent commit's loop cut.  Most runs go through the CLI's list mode: one process and one filter per configuration for
all files of a test.  The carry between two contexts is also checked call by call."""
import ctypes as C
import gzip
import json
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import fastqchunk as F
from tests import harness as H
from tests import readsets as R
from tests import seqgen
from tests.test_bam_subset import EOF_BLOCK, bgzf, bgzf_fancy, build_bam, gunzip_members, make_reads
from tests.test_gpu_bam_device import mutation_files_70
from tests.test_read_routes_multi_cpu import build_cli

pytestmark = pytest.mark.gpu
FLAGS = ["-x", "0", "-l", "18", "-y", "0.8", "-k", "10", "-d", "10"]
GOLDEN = ["fastq_subset.fq", "fastq_subset_blanklines.fq", "fastq_subset_crlf.fq", "fastq_subset_large.fq",
          "fastq_subset_realistic.fq", "fastq_subset_threshold.fq"]
# (name, --device or --host, --devices)
CONFIGS = [("host", "--host", None), ("one", "--device", "0"), ("two", "--device", "0,0"), ("three", "--device", "0,0,0")]


@pytest.fixture(scope="module")
def mcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "read_routes_multi_cli")


def run_each(mcli, root, tag, mode, entries, route, devices, extra, timeout=300):
    """entries: (name, bytes, via stdin) each -> {name: ("ok", result struct text, output) or ("err", message, bytes written
    before it)}, all through one process."""
    d = root / tag
    d.mkdir()
    lines = []
    for name, data, via_stdin in entries:
        (d / name).write_bytes(data)
        lines.append(("<" if via_stdin else "") + str(d / name) + "\n")
    (d / "list.txt").write_text("".join(lines))
    cmd = [mcli, mode, route, "--each", str(d / "list.txt")] + (["--devices", devices] if devices else []) + list(extra)
    r = subprocess.run(cmd, stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-500:])
    out = {}
    for name, _, _ in entries:
        ok, err = d / (name + ".ok"), d / (name + ".err")
        assert ok.exists() != err.exists(), (tag, name)
        out[name] = ("ok", ok.read_text(), (d / (name + ".out")).read_bytes()) if ok.exists() else \
            ("err", err.read_text(), (d / (name + ".partial")).read_bytes())
    return out


def run_one(mcli, mode, path, route, devices, extra, timeout=300):
    """One input through the CLI's single mode -> (CompletedProcess, the JSON line or None)."""
    cmd = [mcli, mode, route] + (["--devices", devices] if devices else []) + list(extra) + [str(path)]
    r = subprocess.run(cmd, stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout)
    return r, (json.loads(r.stderr.decode().splitlines()[-1]) if r.returncode == 0 else None)


def encoded(texts):
    """Every text as a plain file, bgzipped (small members: several per chunk), plain-gzipped and on stdin."""
    entries = []
    for i, (name, text) in enumerate(sorted(texts.items())):
        tag = "t%02d" % i
        entries += [(tag + ".plain", text, False), (tag + ".bgzf", bgzf(text, 3000), False), (tag + ".gzip", gzip.compress(text, 6), False),
                    (tag + ".stdin", text, True)]
    return entries


def fastq_texts():
    texts = {"golden " + g: open(H.golden_path("testFiles/" + g), "rb").read() for g in GOLDEN}
    texts.update(("edge " + k, v) for k, v in F.edge_cases().items())
    texts["generated lf"] = F.reads_text(81, 300)
    texts["generated crlf"] = F.reads_text(82, 300, eol=b"\r\n")
    return texts


@pytest.fixture(scope="module")
def fastq_case(mcli, tmp_path_factory):
    """The inputs in their four encodings and their results on the host route: computed once."""
    root = tmp_path_factory.mktemp("fastq")
    entries = encoded(fastq_texts())
    return root, entries, run_each(mcli, root, "host", "--fastq-subset", entries, "--host", None, FLAGS)


@pytest.mark.parametrize("chunk", [64, 257, 4096])
@pytest.mark.parametrize("tag,devices", [(t, d) for t, _, d in CONFIGS[1:]])
def test_fastq_byte_for_byte(mcli, fastq_case, tag, devices, chunk):
    """1, 2 and 3 contexts against the host route, so against each other.  Records straddle contexts at every size, and at 64
    and 257 bytes most records exceed a chunk."""
    root, entries, host = fastq_case
    got = run_each(mcli, root, "%s_%d" % (tag, chunk), "--fastq-subset", entries, "--device", devices,
                   FLAGS + ["--reads-per-batch", "7", "--chunk-bytes", str(chunk)])
    for name, _, _ in entries:
        assert got[name][0] == "ok", (name, got[name][1])
        assert got[name] == host[name], (name, got[name][:2], host[name][:2])
    assert any(len(v[2]) > 1000 for v in got.values())


def malformed():
    cases = {name: text for name, (text, _, _) in F.error_cases().items()}
    cases["fastq_malformed.fq"] = open(H.golden_path("testFiles/fastq_malformed.fq"), "rb").read()
    # the record that is not valid in the first, a middle and the last of many chunks
    gen = random.Random(19)
    good = [F.record_text(b"g%d" % i, F.random_read(gen, 60 + i, telomeric=i % 2 == 0)) for i in range(24)]
    for where, at in (("first", 0), ("middle", 11), ("last", 23)):
        recs = list(good)
        recs[at] = good[at].replace(b"\n+\n", b"\n-\n", 1) if at else good[at][:-2] + b"\n"
        cases["many chunks, the %s" % where] = b"".join(recs)
    return cases


def test_malformed_fastq_fails_alike(mcli, tmp_path):
    cases = malformed()
    entries = [("bad%02d.fq" % i, text, False) for i, (_, text) in enumerate(sorted(cases.items()))]
    extra = ["-x", "0", "-l", "6", "--chunk-bytes", "257", "--reads-per-batch", "2"]
    one = run_each(mcli, tmp_path, "one", "--fastq-subset", entries, "--device", "0", extra)
    three = run_each(mcli, tmp_path, "three", "--fastq-subset", entries, "--device", "0,0,0", extra)
    host = run_each(mcli, tmp_path, "host", "--fastq-subset", entries, "--host", None, extra[:4])
    expected = dict(F.error_cases())
    for (name, _, _), (case, text) in zip(entries, sorted(cases.items())):
        assert one[name][0] == "err" and three[name] == one[name], (case, three[name][:2], one[name][:2])
        if case in expected:
            _, kind, at = expected[case]
            assert three[name][1] == "FASTQ record %d: %s\n" % (at + 1, F.MESSAGES[kind]), case
        else:                                                       # (one and several contexts share their steps: the host route's message)
            assert host[name][0] == "err" and three[name][1] == host[name][1], (case, three[name][1], host[name][1])
    assert any(len(v[2]) > 0 for v in three.values())              # (something was written before some of the failures)


@pytest.fixture(scope="module")
def two_kb():
    """3 000 reads of 2 kb and one record without SEQ: nine 1 MiB chunks.  -> (header, records, the BAM)"""
    rng = np.random.default_rng(77)
    reads = []
    for i in range(3000):
        s = bytearray(seqgen.random_dna(rng, 2000).tobytes())
        if i % 7 == 0:
            s[:600] = b"TTAGGG" * 100
        reads.append(("k%d" % i, s.decode()))
    return build_bam(reads + [("none", "")], 65280)


def bam_inputs(two_kb):
    gen = random.Random(5)
    rng = np.random.default_rng(123)
    reads = make_reads()
    inputs = {"reads.bam": build_bam(reads, 60000)[2]}
    big = bytearray(seqgen.random_dna(rng, 1_400_000).tobytes())
    t = seqgen.repeat_array("CCCTAA", 2000).tobytes()
    big[-len(t):] = t
    large = list(reads)
    large.insert(200, ("big_telomeric", big.decode()))
    large.insert(300, ("big_plain", seqgen.random_dna(rng, 1_200_000).tobytes().decode()))
    header, records, _ = build_bam(large, 60000)
    inputs["large_records.bam"] = bgzf_fancy(header + b"".join(records), 30011, gen)
    short = []
    for i in range(20000):
        n = int(rng.integers(100, 301))
        short.append(("s%d" % i, ("TTAGGG" * 60)[:n] if i % 50 == 0 else seqgen.random_dna(rng, n).tobytes().decode()))
    inputs["short_reads.bam"] = build_bam(short, 60000)[2]
    inputs["no_eof.bam"] = build_bam(reads[:8], 60000)[2][:-len(EOF_BLOCK)]
    inputs["garbage.bam"] = bgzf(b"NOTBAM" + b"\0" * 100, 60000)
    header, records, inputs["two_kb.bam"] = two_kb
    # a record that is not valid in a later chunk: what was written before it
    records = records[:1500]
    bad = bytearray(records[1200])
    struct.pack_into("<i", bad, 0, 7)
    inputs["bad_record.bam"] = bgzf(header + b"".join(records[:1200]) + bytes(bad) + b"".join(records[1201:]), 65280)
    return inputs


@pytest.fixture(scope="module")
def bam_case(mcli, tmp_path_factory, two_kb):
    """The inputs, and their results on the host route and on one context (index walk): computed once."""
    root = tmp_path_factory.mktemp("bam")
    entries = [(name, data, False) for name, data in sorted(bam_inputs(two_kb).items())]
    extra = ["-l", "42", "--chunk-bytes", str(1 << 20), "--reads-per-batch", "997"]
    host = run_each(mcli, root, "host", "--bam-subset", entries, "--host", None, ["-l", "42"], timeout=600)
    one = run_each(mcli, root, "one", "--bam-subset", entries, "--device", "0", extra + ["--walk", "index"], timeout=600)
    return root, entries, extra, host, one


def test_bam_one_context_is_the_host_route(bam_case):
    _, entries, _, host, one = bam_case
    for name, _, _ in entries:
        assert one[name][0] == host[name][0], (name, one[name][:2], host[name][:2])
        if one[name][0] == "ok":
            assert one[name] == host[name], name
    assert [n for n, _, _ in entries if one[n][0] == "err"] == ["bad_record.bam", "garbage.bam"]
    assert "\"missingEofBlock\": true" in one["no_eof.bam"][1] and len(gunzip_members(one["two_kb.bam"][2])) > 500_000


@pytest.mark.parametrize("walk", ["index", "serial"])
@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
def test_bam_byte_for_byte(mcli, bam_case, devices, walk):
    root, entries, extra, _, one = bam_case
    got = run_each(mcli, root, "n%d_%s" % (len(devices.split(",")), walk), "--bam-subset", entries, "--device", devices, extra + ["--walk", walk], timeout=600)
    for name, _, _ in entries:
        assert got[name] == one[name], (name, got[name][:2], one[name][:2])


def test_bam_mutation_slice_on_two_contexts(mcli, tmp_path):
    entries = [("m%03d.bam" % i, data, False) for i, data in enumerate(mutation_files_70())]
    extra = ["-x", "0", "-l", "18"]
    host = run_each(mcli, tmp_path, "host", "--bam-subset", entries, "--host", None, extra)
    one = run_each(mcli, tmp_path, "one", "--bam-subset", entries, "--device", "0", extra)
    two = run_each(mcli, tmp_path, "two", "--bam-subset", entries, "--device", "0,0", extra)
    for name, _, _ in entries:
        assert two[name] == one[name], (name, two[name][:2], one[name][:2])
        assert two[name][0] == host[name][0], (name, two[name][:2], host[name][:2])
        if two[name][0] == "ok":
            assert two[name] == host[name], name
    assert sum(v[0] == "ok" for v in two.values()) >= 5 and sum(v[0] == "err" for v in two.values()) >= 20


def with_bases(text):
    return sum(1 for r in F.ref_walk(text, True)[0] if r[2] > r[4])


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
def test_every_context_works(mcli, tmp_path, two_kb, devices):
    """Fails without the feature: on one context's code only context 0 ever judges."""
    n = len(devices.split(","))
    text = F.reads_text(83, 300)
    for kind, data in (("plain", text), ("bgzf", bgzf(text, 3000)), ("gzip", gzip.compress(text, 6))):
        p = tmp_path / ("reads." + kind)
        p.write_bytes(data)
        r, js = run_one(mcli, "--fastq-subset", p, "--device", devices, FLAGS + ["--chunk-bytes", "4096"])
        assert r.returncode == 0, r.stderr[-300:]
        ctxs = js["contexts"]
        chunks = [c["chunks"] for c in ctxs]
        assert len(ctxs) == n and sum(chunks) >= len(text) // 4096 >= n, (kind, chunks)
        assert all(c["recordsJudged"] > 0 for c in ctxs), (kind, ctxs)
        assert sum(c["recordsJudged"] for c in ctxs) == with_bases(text) and js["result"]["total"] == 300
        assert max(chunks) - min(chunks) <= 1, (kind, chunks)
        assert sum(c["bytesReceived"] for c in ctxs) == len(text)
    p = tmp_path / "reads.bam"
    p.write_bytes(two_kb[2])
    for walk in ("index", "serial"):
        r, js = run_one(mcli, "--bam-subset", p, "--device", devices, ["--chunk-bytes", str(1 << 20), "--walk", walk])
        assert r.returncode == 0, r.stderr[-300:]
        ctxs = js["contexts"]
        chunks = [c["chunks"] for c in ctxs]
        assert len(ctxs) == n and sum(chunks) >= 6, chunks
        assert all(c["recordsJudged"] > 0 for c in ctxs), ctxs
        assert sum(c["recordsJudged"] for c in ctxs) == 3000 and js["result"]["totalRecords"] == 3001
        assert js["result"]["missingSequenceRecords"] == 1
        assert max(chunks) - min(chunks) <= 1, chunks


# What the build of the commit before the one set of chunk steps (2b8e572, whose one context ran a loop of its own) reports as
# `chunks` on one context for the inputs of test_one_context_pays_nothing_for_the_ring, same flags.
PARENT_CHUNKS = {"plain": 31, "bgzf": 42, "gzip": 31, "index": 9, "serial": 9}


def test_one_context_pays_nothing_for_the_ring(mcli, tmp_path, two_kb):
    """The figures of one context: every chunk comes in place (no staging region, no commit, no wait for a turn), in the chunks
    the loop of the parent commit cut."""
    def one_context(mode, path, extra, judged, received, chunks):
        r, js = run_one(mcli, mode, path, "--device", "0", extra)
        assert r.returncode == 0, r.stderr[-300:]
        assert len(js["contexts"]) == 1, js
        c = js["contexts"][0]
        print(path.name, extra[-1], c)
        assert c["msCommit"] == 0.0 and c["msCarryWait"] == 0.0, c
        assert c["recordsJudged"] == judged and c["bytesReceived"] == received, c
        assert c["chunks"] == chunks, c
        return js

    text = F.reads_text(83, 300)
    for kind, data in (("plain", text), ("bgzf", bgzf(text, 3000)), ("gzip", gzip.compress(text, 6))):
        p = tmp_path / ("reads." + kind)
        p.write_bytes(data)
        js = one_context("--fastq-subset", p, FLAGS + ["--chunk-bytes", "4096"], with_bases(text), len(text), PARENT_CHUNKS[kind])
        assert js["result"]["total"] == 300
    header, records, bam = two_kb
    p = tmp_path / "reads.bam"
    p.write_bytes(bam)
    for walk in ("index", "serial"):
        js = one_context("--bam-subset", p, ["--chunk-bytes", str(1 << 20), "--walk", walk], 3000, len(header) + sum(map(len, records)),
                         PARENT_CHUNKS[walk])
        assert js["result"]["totalRecords"] == 3001


def test_general_pattern_set_on_two_contexts(mcli, tmp_path):
    """-p TTAGGG,TTAGG: a set the tiled kernel does not take, through both routes."""
    flags = R.SETS[0]
    reads = R.reads_for(flags)
    kept = sum(R.oracle_passes(flags))
    assert 0 < kept < len(reads)
    fq = tmp_path / "general.fq"
    fq.write_bytes(R.fastq_text(reads))
    bam = tmp_path / "general.bam"
    bam.write_bytes(build_bam([("r%d" % i, r.decode()) for i, r in enumerate(reads)], 60000)[2])
    for mode, path, extra in (("--fastq-subset", fq, ["--chunk-bytes", "4096"]), ("--bam-subset", bam, ["--chunk-bytes", str(1 << 20)])):
        outs = {}
        for tag, route, devices in CONFIGS[:3]:
            r, js = run_one(mcli, mode, path, route, devices, flags.split() + (extra if route == "--device" else []))
            assert r.returncode == 0, (mode, tag, r.stderr[-300:])
            outs[tag] = (r.stdout, js["result"])
        assert outs["two"] == outs["one"] == outs["host"], mode
        assert outs["two"][1].get("kept", outs["two"][1].get("passedRecords")) == kept


def test_overflow_on_a_later_context(mcli, tmp_path):
    """The dense set that overflows the general kernels' tile slots, its reads behind a chunk of plain ones: on two contexts the
    batch that regrows and rescans is context 1's."""
    rng = np.random.default_rng(23)
    filler = [R.random_bases(rng, 3000) for _ in range(11)]
    text = R.fastq_text(filler + R.overflow_reads())
    chunk = 1 << 16
    assert len(R.fastq_text(filler)) > chunk and text.index(b"A" * 9000) > chunk
    p = tmp_path / "overflow.fq"
    p.write_bytes(text)
    outs = {}
    for tag, route, devices in CONFIGS[:3]:
        r, js = run_one(mcli, "--fastq-subset", p, route, devices, R.OVERFLOW_SET.split() + (["--chunk-bytes", str(chunk)] if route == "--device" else []))
        assert r.returncode == 0, (tag, r.stderr[-300:])
        outs[tag] = (r.stdout, js["result"])
        if tag == "two":
            assert js["contexts"][1]["recordsJudged"] > 0
    assert outs["two"] == outs["one"] == outs["host"] and outs["two"][1]["kept"] >= 5


def test_carry_between_two_contexts_at_every_cut():
    """ts_chunk_carry_over from a chunk of one context to a chunk of another, then staged bytes committed behind the carry:
    every cut of a 200-byte text against Python slicing; the source keeps its bytes."""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    L = K.lib()
    opts = H.parse_cli("--fastq-subset -l 42")
    a, b = ta.ReadTelomereFilter(user_input(opts, device=0)), ta.ReadTelomereFilter(user_input(opts, device=0))
    src, dst = F.Chunk(a._ctx.ptr, 64, 64), F.Chunk(b._ctx.ptr, 64, 64)
    try:
        text = bytes(random.Random(3).randrange(256) for _ in range(200))
        staged = bytes(random.Random(4).randrange(256) for _ in range(333))
        src.upload(text)
        for cut in range(len(text) + 1):
            assert L.ts_chunk_carry_over(dst.ptr, src.ptr, cut, None) == K.TS_OK, L.ts_last_error(b._ctx.ptr)
            assert dst.size() == len(text) - cut and dst.read(0, dst.size()) == text[cut:], cut
            part = staged[:cut % 7 * 50]
            for piece in (part[:len(part) // 3], part[len(part) // 3:]):                  # (staged in two calls)
                assert L.ts_chunk_stage_upload(dst.ptr, piece, len(piece), None) == K.TS_OK, L.ts_last_error(b._ctx.ptr)
            assert L.ts_chunk_staged(dst.ptr) == len(part) and dst.size() == len(text) - cut
            assert L.ts_chunk_commit(dst.ptr, None) == K.TS_OK, L.ts_last_error(b._ctx.ptr)
            assert L.ts_chunk_staged(dst.ptr) == 0
            assert dst.read(0, dst.size()) == text[cut:] + part, cut
            assert src.read(0, src.size()) == text, cut
        # members staged by two inflate calls, committed behind a carry
        plain = F.reads_text(5, 40)
        first, second = plain[:5000], plain[5000:9000]
        assert L.ts_chunk_carry_over(dst.ptr, src.ptr, 150, None) == K.TS_OK
        big = F.Chunk(b._ctx.ptr, 1 << 16, 64)
        try:
            assert L.ts_chunk_carry_over(big.ptr, src.ptr, 150, None) == K.TS_OK
            at = 0
            for piece in (first, second):
                comp = bgzf(piece, 1777)[:-len(EOF_BLOCK)]
                blocks, pos, made = [], 0, 0
                while pos < len(comp):
                    total = struct.unpack_from("<H", comp, pos + 16)[0] + 1
                    crc, isize = struct.unpack_from("<II", comp, pos + total - 8)
                    blocks.append((pos + 18, total - 26, isize, crc, at + made))
                    made += isize
                    pos += total
                arr = (K.BgzfBlock * len(blocks))()
                for i, (s, pl, isz, crc, d) in enumerate(blocks):
                    arr[i].src_off, arr[i].payload_len, arr[i].isize, arr[i].crc, arr[i].dst_off = s, pl, isz, crc, d
                assert L.ts_chunk_stage_inflate(big.ptr, comp, len(comp), arr, len(blocks), None) == K.TS_OK, L.ts_last_error(b._ctx.ptr)
                status = K.BgzfStatus()
                assert L.ts_bam_chunk_status(big.ptr, C.byref(status)) == K.TS_OK and status.code == 0
                at += made
            assert L.ts_chunk_staged(big.ptr) == len(first) + len(second)
            assert L.ts_chunk_commit(big.ptr, None) == K.TS_OK
            assert big.read(0, big.size()) == text[150:] + first + second
        finally:
            big.close()
    finally:
        src.close()
        dst.close()
        a.close()
        b.close()
