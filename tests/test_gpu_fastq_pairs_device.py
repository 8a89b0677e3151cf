"""Interleaved paired FASTQ as a whole through tests/cpp/fastq_pairs_cli.cpp: the device route (fastqSubsetPairedDevice) against
the host route (fastqSubsetPaired) of the same binary on the same input, and both against the rule's plain-Python statement
(tests/fastqpairs.py: ref_paired_subset) with the CPU oracle's read filter and block calls — output, statistics line, block
report, and for the error inputs the message and what was written before it.  Inputs go through --each, many files per process,
so a test opens a handful of processes; every process is one bounded step.  The two new stages are compared one by one in
tests/test_gpu_fastq_pairs_chunk.py."""
import os
import subprocess

import pytest

from tests import fastqchunk as F
from tests import fastqpairs as P
from tests import harness as H
from tests import readblocks as RB
from tests import readsets
from tests.backends import OracleReadFilter
from tests.test_fastq_chunk_reference_cpu import build_cli as build_unpaired_cli
from tests.test_fastq_pairs_reference_cpu import build_cli
from tests.test_gpu_fasta_reads_device import compare, encodings, run_each

pytestmark = pytest.mark.gpu
KINDS = ("plain", "bgzf", "gzip", "stdin")


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "fastq_pairs_cli")


def expected(text, flags):
    """What every route must answer for a complete text: ("ok", bytes, statistics line, report) or ("err", what is written before
    the failure, message, the report of that)."""
    out, stats, msg, judged = P.ref_paired_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset " + flags)))
    # (the filter folds case before it scans; the oracle's segment scan is given the folded read)
    report, _ = RB.ref_report([(n, s.upper()) for n, s in judged], RB.read_oracle(flags))
    return ("err", out, msg, report) if msg else ("ok", out, P.figures(stats), report)


def set_pairs(flags):
    """The set's reads in their given order as pairs, and behind every eleventh pair a pair whose second mate has no bases: its
    first mate is a read that passes and one that fails, in turn -> (reads, the kinds of pair among them)"""
    reads, passes = readsets.reads_for(flags), readsets.oracle_passes(flags)
    assert len(reads) % 2 == 0
    yes, no = passes.index(True), passes.index(False)
    out, kinds, lone = [], set(), []
    for j in range(len(reads) // 2):
        out += reads[2 * j:2 * j + 2]
        kinds.add((bool(passes[2 * j]), bool(passes[2 * j + 1])))
        if j % 11 == 4:
            first = (yes, no)[len(lone) % 2]
            out += [reads[first], b""]
            lone.append(bool(passes[first]))
    assert set(lone) == {True, False}
    return out, kinds


def small_pairs(flags):
    """Ten pairs of the same reads for chunks of 256 bytes: the set's first pair of each kind (both pass, first only, second only,
    neither), in input order, and its reads of 1 to 16 bases, which all fail."""
    reads, passes = readsets.reads_for(flags), readsets.oracle_passes(flags)
    first = {}
    for j in range(len(reads) // 2):
        first.setdefault((bool(passes[2 * j]), bool(passes[2 * j + 1])), j)
    assert len(first) == 4
    pick = [i for j in sorted(first.values()) for i in (2 * j, 2 * j + 1)] + list(range(60, 72))
    assert all(len(reads[i]) <= 16 and not passes[i] for i in pick[8:])
    return [reads[i] for i in pick]


@pytest.mark.parametrize("s", range(len(readsets.SETS)), ids=readsets.SET_IDS)
def test_read_sets_as_pairs(dcli, tmp_path, s):
    """The reads of a pattern set as pairs, named three ways (p<j>/1 and /2; p<j> 1:N:0 and 2:N:0; bare equal names), as a plain
    file, bgzipped, gzipped and on stdin (the first set: every name style in every encoding, and a CRLF variant; the others: a
    rotating encoding per style), through chunks of 4 096 and 65 536 bytes, 2, 37 (38) and the default reads per batch, one, two and
    three contexts; and ten pairs of them through chunks of 256 bytes, where nearly every chunk ends between mates and many hold
    no whole pair: device == host == the statement."""
    flags = readsets.SETS[s]
    reads, kinds = set_pairs(flags)
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    files, want, small = {}, {}, {}
    for i, style in enumerate(P.STYLES):
        text = P.paired_text(reads, style)
        w = expected(text, flags)
        assert w[0] == "ok" and w[1] and len(w[1]) < len(text) and w[3]
        for kind, entry in encodings(tmp_path, style, text, KINDS if s == 0 else (KINDS[(s + i) % 4],)).items():
            files[style, kind], want[style, kind] = entry, w
        text = P.paired_text(small_pairs(flags), style)
        p = tmp_path / ("small.%s" % style)
        p.write_bytes(text)
        small[style], want["small", style] = str(p), expected(text, flags)
        assert want["small", style][2] == P.figures((20, 6))
    if s == 0:
        text = P.paired_text(reads, "slash", b"\r\n")
        files["slash", "crlf"], want["slash", "crlf"] = encodings(tmp_path, "crlf", text, ("plain",))["plain"], expected(text, flags)
        assert want["slash", "crlf"][2] == want["slash", "plain"][2] and want["slash", "crlf"][1] == want["slash", "plain"][1].replace(b"\n", b"\r\n")
    runs = {"host": ["--host", "--chunk-bytes", "65536", "--reads-per-batch", "37"],
            "device, chunks of 4096, 37 per batch, three contexts": ["--device", "--chunk-bytes", "4096", "--reads-per-batch", "37", "--contexts", "3"],
            "device, chunks of 65536, one context": ["--device", "--chunk-bytes", "65536"]}
    if s == 0:
        runs["device, chunks of 4096, 2 per batch, two contexts"] = ["--device", "--chunk-bytes", "4096", "--reads-per-batch", "2", "--contexts", "2"]
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(files.values()), route + flags.split())
        for key, entry in files.items():
            compare(got[entry], want[key], (who, key))
    runs = {"device, chunks of 256, %d contexts" % (1 + s % 3): ["--device", "--chunk-bytes", "256", "--reads-per-batch", "2", "--contexts", str(1 + s % 3)],
            "host, blocks of 256": ["--host", "--chunk-bytes", "256", "--reads-per-batch", "3"]}
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(small.values()), route + flags.split())
        for style, entry in small.items():
            compare(got[entry], want["small", style], (who, style))


FLAGS = "-l 42"
T = b"TTAGGG" * 20
N = b"ACGTCA" * 20


def rec(name, seq, eol=b"\n"):
    return F.record_text(name, seq, eol=eol)


def error_inputs():
    """name -> text: every error of the rule, each with kept pairs in front of it (and pairs that are not kept among them)."""
    k = lambda j, a=T, b=N: rec(b"k%d/1" % j, a) + rec(b"k%d/2" % j, b)     # noqa: E731
    good = k(0) + k(1, N, N) + k(2, N, T) + k(3, T, T) + k(4, N, N) + rec(b"e 1", T) + rec(b"e 2", b"")
    bad = rec(b"m/1", T) + rec(b"n/2", T)
    cases = {
        "odd record count": good + rec(b"z/1", T),
        "mismatch in the middle": good + bad + k(5), "mismatch last": good + bad,
        "record error behind a mismatch": good + bad + k(5) + F._damage(F.BAD_HEADER, b"bad") + k(6),
        "mismatch behind a record error": good + rec(b"o", T) + F._damage(F.BAD_LENGTHS, b"bad") + bad,
        "truncated first mate": good + b"@cut\n" + T + b"\n+", "truncated second mate": good + rec(b"cut", T) + b"@cut\n" + T,
    }
    for kind in (F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS):
        cases["%s at the first mate" % F.MESSAGES[kind]] = good + F._damage(kind, b"bad") + rec(b"bad", T) + k(7)
        cases["%s at the second mate" % F.MESSAGES[kind]] = good + rec(b"bad", T) + F._damage(kind, b"bad") + k(7)
    return cases


def test_error_inputs_hold_what_they_name():
    """(without a device) the error inputs hold what they name: the message, and kept pairs in front of it."""
    want = {name: expected(text, FLAGS) for name, text in error_inputs().items()}
    written = b"".join(rec(b"k%d/%d" % (j, m), s) for j, a, b in ((0, T, N), (2, N, T), (3, T, T)) for m, s in ((1, a), (2, b))) + rec(b"e 1", T) + rec(b"e 2", b"")
    assert all(w[0] == "err" and w[1] == written and w[3].count(b"\n") >= 5 for w in want.values())
    assert want["odd record count"][2] == P.UNPAIRED
    assert want["mismatch in the middle"][2] == want["mismatch last"][2] == want["record error behind a mismatch"][2] == P.name_error(6)
    assert want["mismatch behind a record error"][2] == P.record_error(F.BAD_LENGTHS, 13)
    assert want["truncated first mate"][2] == P.record_error(F.TRUNCATED, 12) and want["truncated second mate"][2] == P.record_error(F.TRUNCATED, 13)
    for kind in (F.BAD_HEADER, F.BAD_SEPARATOR, F.BAD_LENGTHS):
        assert want["%s at the first mate" % F.MESSAGES[kind]][2] == P.record_error(kind, 12)
        assert want["%s at the second mate" % F.MESSAGES[kind]][2] == P.record_error(kind, 13)


@pytest.mark.parametrize("contexts", [1, 2, 3])
def test_error_inputs(dcli, tmp_path, contexts):
    """Every error input through chunks of 256 bytes (a pair is ~ 500: the chunk grows, and most chunks end inside a pair) and of
    65 536, 2 and 37 reads per batch, on one, two and three contexts, and the host route: message and partial output, the block
    report of the pairs written included, are the statement's on every route."""
    entries, want = {}, {}
    for i, (name, text) in enumerate(sorted(error_inputs().items())):
        p = tmp_path / ("case%02d.fq" % i)
        p.write_bytes(text)
        entries[name], want[name] = str(p), expected(text, FLAGS)
    runs = {"device, chunks of %d, %d per batch" % (c, r): ["--device", "--contexts", str(contexts), "--chunk-bytes", str(c), "--reads-per-batch", str(r)]
            for c, r in ((256, 2), (65536, 37), (700, 37))}
    if contexts == 1:
        runs["host"] = ["--host", "--chunk-bytes", "256", "--reads-per-batch", "2"]
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(entries.values()), route + FLAGS.split())
        for name, entry in entries.items():
            compare(got[entry], want[name], (who, name))
    if contexts == 1:                                               # ... and two of them through the other sources
        for name in ("odd record count", "mismatch in the middle"):
            files = encodings(tmp_path, "src", error_inputs()[name])
            got = run_each(dcli, tmp_path, list(files.values()), ["--device", "--chunk-bytes", "256"] + FLAGS.split())
            for kind, entry in files.items():
                compare(got[entry], want[name], (name, kind))


def test_refused_inputs(dcli, tmp_path):
    cases = {"empty": b"", "blank first": b"\n" + rec(b"a", T) + rec(b"a", T), "fasta": b">a\nACGT\n"}
    entries = {}
    for i, (name, text) in enumerate(cases.items()):
        p = tmp_path / ("refused%d.fq" % i)
        p.write_bytes(text)
        entries[name] = str(p)
    for route in (["--device", "--chunk-bytes", "256"], ["--device", "--contexts", "2"], ["--host"]):
        got = run_each(dcli, tmp_path, list(entries.values()), route + FLAGS.split())
        assert got[entries["empty"]] == ("err", b"", P.EMPTY, b""), route
        assert got[entries["blank first"]] == ("err", b"", P.NO_HEADER, b"") == got[entries["fasta"]], route


def test_every_record_passes_equals_the_unpaired_route(dcli, tmp_path, tmp_path_factory):
    """An input of which every record passes: the paired routes write what the unpaired device route writes, byte for byte; and the
    single-input form of the program: the subset on stdout, the statistics line on stderr, exit status 1 and "Error: ..."."""
    ucli = build_unpaired_cli(tmp_path_factory.mktemp("cpp") / "fastq_device_cli")
    text = b"".join(rec(b"a%d/1" % j, T + b"ACGT" * j) + rec(b"a%d/2" % j, b"CCCTAA" * (20 + j), eol=b"\r\n" if j % 5 == 0 else b"\n") for j in range(40))
    p = tmp_path / "all.fq"
    p.write_bytes(text)
    u = subprocess.run([ucli, "--fastq-subset", "--device"] + FLAGS.split() + ["--fastq-chunk-bytes", "4096", str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert u.returncode == 0 and u.stdout == text, u.stderr[-300:]
    want = expected(text, FLAGS)
    assert want[:3] == ("ok", text, P.figures((80, 80)))
    for route in (["--device", "--chunk-bytes", "4096"], ["--device", "--chunk-bytes", "4096", "--contexts", "2", "--reads-per-batch", "7"], ["--host"]):
        r = subprocess.run([dcli] + route + FLAGS.split() + [str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout == u.stdout and r.stderr.decode().splitlines()[-1] == want[2], (route, r.stderr[-300:])
    bad = tmp_path / "bad.fq"
    bad.write_bytes(text + rec(b"z/1", T))
    for route in ("--device", "--host"):
        r = subprocess.run([dcli, route] + FLAGS.split() + [str(bad)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == text and r.stderr.decode().splitlines()[-1] == "Error: " + P.UNPAIRED, route
