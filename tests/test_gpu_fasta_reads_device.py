"""The FASTA read subset as a whole through tests/cpp/fasta_subset_cli.cpp: the device route (fastaSubsetDevice) against the host
route (fastaSubset) of the same binary on the same input, byte for byte — output, statistics line, block report, and for the two
error inputs the message — and both against the rule's plain-Python restatement (tests/fastareads.py: ref_subset) with the CPU
oracle's read filter and block calls.  Inputs go through --each, many files per process, so a test opens a handful of processes;
every process is one bounded step.  The stages are compared one by one in tests/test_gpu_fasta_reads_chunk.py."""
import glob
import gzip
import os
import subprocess

import pytest

from tests import fastareads as R
from tests import harness as H
from tests import readblocks as RB
from tests import readsets
from tests.backends import OracleReadFilter
from tests.test_bam_subset import bgzf
from tests.test_fasta_reads_reference_cpu import build_cli

pytestmark = pytest.mark.gpu
CHUNKS = (4096, 65536)
COMMITTED = sorted(glob.glob(os.path.join(H.GOLDEN, "testFiles", "*.fa")))


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "fasta_subset_cli")


def encodings(d, tag, text, kinds=("plain", "bgzf", "gzip", "stdin")):
    """The text as a plain file, bgzipped (members of 3 000 bytes: several per chunk), plain-gzipped, and the plain file on stdin:
    name -> the line of an --each list."""
    made = {"plain": lambda: text, "bgzf": lambda: bgzf(text, 3000), "gzip": lambda: gzip.compress(text, 6), "stdin": lambda: text}
    out = {}
    for name in kinds:
        p = d / ("%s.%s" % (tag, name))
        p.write_bytes(made[name]())
        out[name] = ("<" if name == "stdin" else "") + str(p)
    return out


def run_each(dcli, d, entries, args, timeout=300):
    """One process over the entries of an --each list, with the block report -> entry -> ("ok", output, the statistics line,
    report) or ("err", what was written before the failure, the message, the report so far).  The result files are removed."""
    lst = d / "list.txt"
    lst.write_text("".join(e + "\n" for e in entries))
    r = subprocess.run([dcli, "--each", str(lst), "--blocks"] + list(args), stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    res = {}
    for e in entries:
        p = e.lstrip("<")
        got = {s: p + s for s in (".out", ".ok", ".err", ".partial", ".blocks") if os.path.exists(p + s)}
        assert set(got) in ({".out", ".ok", ".blocks"}, {".err", ".partial", ".blocks"}), (e, sorted(got), r.stderr[-400:])
        kind = "ok" if ".ok" in got else "err"
        body, note = (".out", ".ok") if kind == "ok" else (".partial", ".err")
        res[e] = (kind, open(got[body], "rb").read(), open(got[note]).read().strip(), open(got[".blocks"], "rb").read())
        for path in got.values():
            os.remove(path)
    return res


def expected(text, flags):
    """What every route must answer for a complete text: ("ok", bytes, statistics line, report) or ("err", b"", message, b"")."""
    out, stats, msg, judged = R.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset " + flags)))
    if msg:
        return ("err", out, msg, b"")
    # (the filter folds case before it scans; the oracle's segment scan is given the folded read)
    report, _ = RB.ref_report([(n, s.upper()) for n, s in judged], RB.read_oracle(flags))
    return ("ok", out, R.figures(stats), report)


def compare(got, want, what):
    assert got[0] == want[0] and got[2] == want[2], (what, got[0], got[2], want[2])
    assert got[1] == want[1], (what, "output", len(got[1]), len(want[1]))
    assert got[3] == want[3], (what, "block report", len(got[3]), len(want[3]))


ALL_SETS = list(zip(readsets.SET_IDS, readsets.SETS)) + [("overflow", readsets.OVERFLOW_SET)]


def set_reads(flags):
    """(reads, names): the set's reads as r0, r1, ... and behind every eleventh a record without bases, e<i>."""
    reads = readsets.overflow_reads() if flags == readsets.OVERFLOW_SET else readsets.reads_for(flags)
    out, names = [], []
    for i, r in enumerate(reads):
        out.append(r)
        names.append(b"r%d" % i)
        if i % 11 == 4:
            out.append(b"")
            names.append(b"e%d some words" % i)
    return reads, out, names


@pytest.mark.parametrize("flags", [f for _, f in ALL_SETS], ids=[i for i, _ in ALL_SETS])
def test_read_sets_every_width_source_and_chunk_size(dcli, tmp_path, flags):
    """The generated reads of every pattern set tests/readsets.py offers (general tips batches; the overflow set regrows and
    rescans), written as FASTA unwrapped, at width 60 and at width 1, as a plain file, bgzipped, gzipped and on stdin, through
    chunks of 4 096 bytes (records straddle chunks, and the longer reads exceed one: the chunk grows; on one context and on
    three) and of 65 536: device == host == the reference; the kept names are the oracle's verdicts on the bare sequences,
    whatever the line width; the records without bases are counted and never kept."""
    reads, with_empty, names = set_reads(flags)
    passes = OracleReadFilter(readsets.options(flags)).filter(reads) if flags == readsets.OVERFLOW_SET else readsets.oracle_passes(flags)
    kept = ["r%d" % i for i, ok in enumerate(passes) if ok]
    assert 0 < len(kept) < len(reads)
    files, want = {}, {}
    for width in (None, 60, 1):
        text = R.reads_text(with_empty, width, b"\r\n" if width == 60 else b"\n", names)
        w = expected(text, flags)
        assert w[0] == "ok" and R.kept_names(w[1]) == kept, width
        assert w[2] == R.figures((len(with_empty), len(kept), len(with_empty) - len(reads))) and w[3].count(b"\n") >= len(kept)
        for kind, entry in encodings(tmp_path, "w%s" % width, text).items():
            files[width, kind], want[width, kind] = entry, w
    runs = {"host": ["--host", "--chunk-bytes", "65536"]}
    for chunk in CHUNKS:
        runs["device, chunks of %d" % chunk] = ["--device", "--chunk-bytes", str(chunk)]
    runs["device, chunks of 4096, three contexts"] = ["--device", "--chunk-bytes", "4096", "--contexts", "3"]
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(files.values()), route + flags.split() + ["--reads-per-batch", "37"])
        for key, entry in files.items():
            compare(got[entry], want[key], (who, key))


def test_committed_fasta_concatenated(dcli, tmp_path):
    """The committed FASTA inputs, one behind the other, as reads under the default flags (the tiled kernel): a mixture, of which
    some records pass and some do not; every source, both chunk sizes, one read and 37 reads per batch, one, two and three
    contexts, and the host route."""
    flags = ""
    text = b"".join(t if t.endswith(b"\n") else t + b"\n" for t in (open(p, "rb").read() for p in COMMITTED))
    want = expected(text, flags)
    total, kept = text.count(b"\n>") + 1, len(R.kept_names(want[1]))
    assert want[0] == "ok" and len(COMMITTED) >= 40 and total >= 44 and 0 < kept < total and want[3]
    files = encodings(tmp_path, "committed", text)
    runs = {"host": ["--host", "--chunk-bytes", "65536", "--reads-per-batch", "37"], "host, one read per batch": ["--host", "--chunk-bytes", "4096", "--reads-per-batch", "1"]}
    for chunk in CHUNKS:
        for rpb in (1, 37):
            for contexts in (1, 2, 3):
                if contexts == 1 or (chunk, rpb) in ((4096, 37), (65536, 1)):
                    runs["device, chunks of %d, %d per batch, %d contexts" % (chunk, rpb, contexts)] = [
                        "--device", "--chunk-bytes", str(chunk), "--reads-per-batch", str(rpb), "--contexts", str(contexts)]
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(files.values()), route)
        for kind, entry in files.items():
            compare(got[entry], want, (who, kind))


def small_inputs():
    """name -> text: the rule's edge cases, inputs with records that have no bases, and the two error inputs."""
    cases = dict(R.edge_cases())
    cases["many records without bases"] = b"".join(b">e%d\n" % i if i % 3 else b">r%d\n%s\n" % (i, b"CCCTAA" * (5 + i)) for i in range(40))
    cases["empty input"] = b""
    cases["no header first"] = b"ACGT\n>a\n" + b"TTAGGG" * 9 + b"\n"
    cases["a blank line first"] = b"\n>a\n" + b"TTAGGG" * 9 + b"\n"
    cases["fastq"] = readsets.fastq_text([b"TTAGGG" * 9])
    return cases


@pytest.mark.parametrize("contexts", [1, 2, 3])
def test_small_inputs_in_chunks_of_256_bytes(dcli, tmp_path, contexts):
    """Every edge case of the rule and the error inputs through chunks of 256 bytes — smaller than the 300-byte name and the
    longer records, so the chunk grows — and of 65 536, one read per batch, on one, two and three contexts: device == host == the
    reference, messages included; nothing depends on the number of contexts."""
    flags = "-l 42"
    entries, want = {}, {}
    for i, (name, text) in enumerate(sorted(small_inputs().items())):
        p = tmp_path / ("case%02d.fa" % i)
        p.write_bytes(text)
        entries[name], want[name] = str(p), expected(text, flags)
    assert want["empty input"] == ("err", b"", R.EMPTY, b"")
    for name in ("no header first", "a blank line first", "fastq"):
        assert want[name] == ("err", b"", R.NO_HEADER, b"")
    assert want["many records without bases"][2].endswith("of 40 records (26 without sequence).") and want["many records without bases"][1]
    assert sum(1 for w in want.values() if w[0] == "ok" and w[1]) >= 20
    runs = {"device, chunks of %d" % c: ["--device", "--contexts", str(contexts), "--chunk-bytes", str(c)] for c in (256, 65536)}
    if contexts == 1:
        runs["host"] = ["--host", "--chunk-bytes", "256"]
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(entries.values()), route + flags.split() + ["--reads-per-batch", "1"])
        for name, entry in entries.items():
            compare(got[entry], want[name], (who, name))
    if contexts == 1:                                               # ... and the error inputs through the other sources
        for name in ("empty input", "fastq"):
            files = encodings(tmp_path, "src", small_inputs()[name])
            got = run_each(dcli, tmp_path, list(files.values()), ["--device", "--chunk-bytes", "256"] + flags.split())
            for kind, entry in files.items():
                compare(got[entry], want[name], (name, kind))


def test_plain_gzip_inflated_on_the_device(dcli, tmp_path, monkeypatch):
    """TS_GZIP_DEVICE=1 (with TS_GZIP_MIN_BYTES=0 and small spans, so that a small file takes that source): the plain-gzipped text
    is decoded on the device by the feed, and the route answers what it answers for the plain file."""
    monkeypatch.setenv("TS_GZIP_DEVICE", "1")
    monkeypatch.setenv("TS_GZIP_MIN_BYTES", "0")
    monkeypatch.setenv("TS_GZIP_SPAN", "4096")
    flags = "-l 42"
    reads, with_empty, names = set_reads(readsets.SETS[0])
    text = R.reads_text(with_empty, 60, b"\n", names)
    want = expected(text, flags)
    assert want[0] == "ok" and want[1]
    p = tmp_path / "reads.fa.gz"
    p.write_bytes(gzip.compress(text, 6))
    for chunk in CHUNKS:
        got = run_each(dcli, tmp_path, [str(p)], ["--device", "--chunk-bytes", str(chunk)] + flags.split())
        compare(got[str(p)], want, chunk)


def test_cli_single_input_and_statistics_line(dcli, tmp_path):
    """Without --each: the subset on stdout, the statistics line on stderr, exit status 1 and "Error: ..." for an error input."""
    text = R.edge_cases()["names"]
    p = tmp_path / "names.fa"
    p.write_bytes(text)
    want = expected(text, "-l 42")
    for route in ("--device", "--host"):
        r = subprocess.run([dcli, route, "-l", "42", str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout == want[1] and r.stderr.decode().splitlines()[-1] == want[2], (route, r.stderr[-300:])
        bad = tmp_path / "bad.fa"
        bad.write_bytes(b"@r\nACGT\n+\nIIII\n")
        r = subprocess.run([dcli, route, str(bad)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().splitlines()[-1] == "Error: " + R.NO_HEADER, route
