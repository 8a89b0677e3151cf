"""--sam-subset as a whole through tests/cpp/sam_device_cli.cpp: the device route (samSubsetDevice) against the host route
(samSubset) of the same binary on the same input, byte for byte — output, statistics, and for a bad input the message and what
was written before it — and both against the rule's plain-Python restatement (tests/samchunk.py: ref_subset) with the CPU
oracle's read filter.  Inputs go through --each, many files per process, so a test opens a handful of processes; every process
is one bounded step.  The stages are compared one by one in tests/test_gpu_sam_chunk.py."""
import gzip
import json
import os
import subprocess

import pytest

from tests import harness as H
from tests import readsets
from tests import samchunk as S
from tests.backends import OracleReadFilter
from tests.test_bam_subset import _kept_names, bgzf, build_bam, gunzip_members, make_reads
from tests.test_cpp_mirror import cli  # noqa: F401  (fixture: builds tests/cpp/manifest_cli.cpp, the bamSubset entry)
from tests.test_sam_chunk_reference_cpu import build_cli

pytestmark = pytest.mark.gpu
CHUNKS = (4096, 65536)
LONG_HEADER = S.HEADER + b"".join(b"@SQ\tSN:contig_%d\tLN:%d\n" % (i, 1000 + i) for i in range(260))      # straddles a 4 096-byte chunk


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "sam_device_cli")


def encodings(d, tag, text):
    """The text as a plain file, bgzipped (small members: several per chunk), plain-gzipped, and the plain file on stdin: name ->
    the line of an --each list."""
    out = {}
    for name, data in (("plain", text), ("bgzf", bgzf(text, 3000)), ("gzip", gzip.compress(text, 6)), ("stdin", text)):
        p = d / ("%s.%s" % (tag, name))
        p.write_bytes(data)
        out[name] = ("<" if name == "stdin" else "") + str(p)
    return out


def run_each(dcli, d, entries, args, timeout=120):
    """One process over the entries of an --each list -> entry -> ("ok", output, the statistics line) or ("err", what was
    written before the failure, the message).  The result files are removed, so that the next run starts clean."""
    lst = d / "list.txt"
    lst.write_text("".join(e + "\n" for e in entries))
    r = subprocess.run([dcli, "--sam-subset", "--each", str(lst)] + list(args), stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    res = {}
    for e in entries:
        p = e.lstrip("<")
        got = {s: p + s for s in (".out", ".ok", ".err", ".partial") if os.path.exists(p + s)}
        assert set(got) in ({".out", ".ok"}, {".err", ".partial"}), (e, sorted(got), r.stderr[-400:])
        kind = "ok" if ".ok" in got else "err"
        body, note = (".out", ".ok") if kind == "ok" else (".partial", ".err")
        res[e] = (kind, open(got[body], "rb").read(), open(got[note]).read().strip())
        for path in got.values():
            os.remove(path)
    return res


def figures(stats):
    headers, total, kept, missing = stats
    return "SAM subset: kept %d of %d records (%d without sequence, %d header lines)." % (kept, total, missing, headers)


def expected(text, flags):
    """What every route must answer for a complete text: ("ok", bytes, statistics line) or ("err", bytes before, message)."""
    out, stats, msg = S.ref_subset(text, OracleReadFilter(H.parse_cli("--fastq-subset " + flags)))
    return ("err", out, msg) if msg else ("ok", out, figures(stats))


ALL_SETS = list(zip(readsets.SET_IDS, readsets.SETS)) + [("overflow", readsets.OVERFLOW_SET)]


@pytest.mark.parametrize("flags", [f for _, f in ALL_SETS], ids=[i for i, _ in ALL_SETS])
def test_read_sets_every_source_and_chunk_size(dcli, tmp_path, flags):
    """The generated reads of every pattern set tests/readsets.py offers (the tiled kernel's sets are the other tests'; these
    take the general tips batch, the mixed-length set -p TTAGGG,TTAGG first), as a plain file, bgzipped, gzipped and on stdin,
    through chunks of 4 096 bytes (the header, lines and records straddle chunks, and the 8 kb reads exceed one) and of 65 536:
    device == host == the reference, and the kept QNAMEs are the oracle's verdicts."""
    reads = readsets.reads_for(flags)
    text = S.reads_text(reads, header=LONG_HEADER)
    want = expected(text, flags)
    assert want[0] == "ok" and len(LONG_HEADER) > 4096 and max(len(r) for r in reads) > 8000
    assert S.kept_names(want[1]) == ["r%d" % i for i, ok in enumerate(readsets.oracle_passes(flags)) if ok]
    files = encodings(tmp_path, "set", text)
    for chunk in CHUNKS:
        args = flags.split() + ["--chunk-bytes", str(chunk), "--reads-per-batch", "37"]
        dev = run_each(dcli, tmp_path, list(files.values()), ["--device"] + args)
        host = run_each(dcli, tmp_path, list(files.values()), ["--host"] + args)
        for kind, entry in files.items():
            assert dev[entry] == host[entry] == want, (kind, chunk, dev[entry][0], dev[entry][2], host[entry][2])


def test_bam_reads_as_sam(cli, dcli, tmp_path):  # noqa: F811
    """make_reads() of tests/test_bam_subset.py as BAM through bamSubset and, converted field by field, as SAM through both SAM
    routes: the same kept names, the same count of records without sequence."""
    reads = make_reads()
    header, records, bam = build_bam(reads, 60000)
    path = tmp_path / "in.bam"
    path.write_bytes(bam)
    r = subprocess.run([cli, "--bam-subset", "-l", "42", str(path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-300:]
    bam_kept = _kept_names(gunzip_members(r.stdout), header)
    assert b"BAM subset: skipped 1 record without SEQ." in r.stderr and 0 < len(bam_kept) < len(reads)
    text = S.bam_to_sam(header + b"".join(records))
    sam = tmp_path / "in.sam"
    sam.write_bytes(text)
    for route in ("--device", "--host"):
        got = run_each(dcli, tmp_path, [str(sam)], [route, "-l", "42", "--chunk-bytes", "65536"], timeout=300)[str(sam)]
        assert got[0] == "ok" and S.kept_names(got[1]) == bam_kept, route
        assert got[2] == figures((2, len(reads), len(bam_kept), 1)), route
        assert got[1].startswith(text[:text.index(b"kat_pass")])


THRESHOLDS = [
    ([], [("short", "TTAGGG" * 6), ("default_pass", "TTAGGG" * 7), ("long", "CCCTAA" * 15), ("fail", "ACGT" * 20)], ["default_pass", "long"]),
    (["-x", "0", "-l", "12", "-y", "1", "-k", "10", "-d", "10"],
     [("one_repeat", "TTAGGG"), ("exact_12", "TTAGGG" * 2), ("flanked_exact", "ACGT" + "CCCTAA" * 2 + "TGCA"), ("exact_18", "TTAGGG" * 3)],
     ["exact_12", "flanked_exact", "exact_18"]),
    (["-x", "0", "-l", "18", "-y", "1", "-k", "10", "-d", "10"],
     [("one_repeat", "TTAGGG"), ("exact_12", "TTAGGG" * 2), ("flanked_exact", "ACGT" + "CCCTAA" * 2 + "TGCA"), ("exact_18", "TTAGGG" * 3)],
     ["exact_18"]),
    (["-x", "0", "-l", "18", "-y", "0.666", "-k", "20", "-d", "10"], [("two_thirds", "TTAGGGAAAAAATTAGGG")], ["two_thirds"]),
    (["-x", "0", "-l", "18", "-y", "0.667", "-k", "20", "-d", "10"], [("two_thirds", "TTAGGGAAAAAATTAGGG")], []),
    (["-c", "CCCTAAA", "-x", "0", "-l", "21", "-y", "1"], [("plant_pass", "TTTAGGG" * 3), ("vertebrate_fail", "TTAGGG" * 4)], ["plant_pass"]),
]


@pytest.mark.parametrize("case", range(len(THRESHOLDS)), ids=["default", "l12", "l18", "y0.666", "y0.667", "plant"])
def test_threshold_known_answers(dcli, tmp_path, case):
    """The known-answer thresholds of test_bam_threshold_known_answers (tests/test_bam_subset.py), as SAM, on both routes."""
    flags, reads, kept = THRESHOLDS[case]
    text = S.HEADER + b"".join(S.sam_line(n.encode(), s.encode(), tags=(b"NM:i:0",)) for n, s in reads)
    p = tmp_path / "t.sam"
    p.write_bytes(text)
    for route in ("--device", "--host"):
        got = run_each(dcli, tmp_path, [str(p)], [route] + flags)[str(p)]
        assert got[0] == "ok" and S.kept_names(got[1]) == kept and got[1].startswith(S.HEADER), (route, got)


@pytest.mark.parametrize("chunk", [100, 65536])
def test_error_cases_fail_alike(dcli, tmp_path, chunk):
    """Every error case of the rule, with LF and CR LF, and the empty input: both routes answer the reference's message with the
    input's line number, and have written the header and the valid records before the bad line, and nothing else."""
    flags = "-x 0 -l 6"
    cases = {}
    for name, (text, _, _) in sorted(S.error_cases().items()):
        cases[name] = text
        cases[name + " (crlf)"] = text.replace(b"\n", b"\r\n")
    cases["empty input"] = b""
    entries, want = {}, {}
    for i, (name, text) in enumerate(sorted(cases.items())):
        p = tmp_path / ("bad%02d.sam" % i)
        p.write_bytes(text)
        entries[name] = str(p)
        want[name] = expected(text, flags)
        assert want[name][0] == "err"
    for name, (_, kind, line) in S.error_cases().items():
        assert want[name][2] == "SAM line %d: %s" % (line + 1, S.MESSAGES[kind])
    assert want["empty input"] == ("err", b"", "SAM input is empty") and any(w[1] for w in want.values())
    args = flags.split() + ["--chunk-bytes", str(chunk), "--reads-per-batch", "2"]
    dev = run_each(dcli, tmp_path, list(entries.values()), ["--device"] + args)
    host = run_each(dcli, tmp_path, list(entries.values()), ["--host"] + args)
    for name, entry in entries.items():
        assert dev[entry] == host[entry] == want[name], (name, dev[entry], host[entry])
    # ... and through the other sources, a case of each kind
    some = ["two errors: the lower one", "a short line borrows no tab", "empty seq before tags", "header after the only record"]
    for name in some:
        files = encodings(tmp_path, "src", cases[name])
        dev = run_each(dcli, tmp_path, list(files.values()), ["--device"] + args)
        for kind, entry in files.items():
            assert dev[entry] == want[name], (name, kind, dev[entry])


@pytest.mark.parametrize("chunk", CHUNKS)
def test_context_counts(dcli, tmp_path, chunk):
    """--devices 0,0 and 0,0,0 (the ring deals the chunks) against one context (every chunk in place) and the host route:
    output, statistics and messages do not depend on the count."""
    flags = "-l 42"
    good = S.generated(21, 150, 30, 1500, header=LONG_HEADER) + S.sam_line(b"long", b"CCCTAA" * 1500)
    crlf = S.generated(22, 80, 30, 900, eol=b"\r\n")
    bad = S.generated(23, 100, 30, 900) + b"short\tline\n" + S.generated(24, 30, header=b"")
    late = S.generated(25, 100, 30, 900) + b"@CO\tlate\n" + S.generated(26, 20, header=b"")
    files, want = {}, {}
    for tag, text in (("good", good), ("crlf", crlf), ("bad", bad), ("late", late), ("headeronly", LONG_HEADER)):
        for kind, entry in encodings(tmp_path, tag, text).items():
            if kind != "gzip":
                files[tag, kind] = entry
                want[tag, kind] = expected(text, flags)
    assert want["good", "plain"][0] == want["headeronly", "plain"][0] == "ok" and want["bad", "plain"][0] == want["late", "plain"][0] == "err"
    args = flags.split() + ["--chunk-bytes", str(chunk), "--reads-per-batch", "97"]
    runs = {"host": ["--host"], "one context": ["--device"], "0,0": ["--device", "--devices", "0,0"], "0,0,0": ["--device", "--devices", "0,0,0"]}
    for who, route in runs.items():
        got = run_each(dcli, tmp_path, list(files.values()), route + args, timeout=300)
        for key, entry in files.items():
            assert got[entry] == want[key], (who, key, got[entry][0], got[entry][2], want[key][2])


# What sam_device_cli of the commit before the shared chunk steps (173634d, with nothing but the --figures switch added) reports
# as `chunks` on one context for the input and flags of test_per_context_figures.
PARENT_CHUNKS = 53


def test_per_context_figures(dcli, tmp_path):
    """--figures on one, two and three contexts: together the contexts judged every record that has a sequence and received every
    byte of the text, each of them judged something and the chunks are dealt evenly; one context takes every chunk in place (no
    commit, no wait for a turn), in the chunks the parent commit cut."""
    text = S.generated(41, 150, 30, 1500)
    recs = S.ref_walk(text, True, True)[0]
    with_seq = sum(1 for r in recs if not r[4] & S.SEQ_IS_STAR)
    assert 0 < with_seq < len(recs)
    p = tmp_path / "reads.sam"
    p.write_bytes(text)
    for devices in ("0", "0,0", "0,0,0"):
        r = subprocess.run([dcli, "--sam-subset", "--device", "--devices", devices, "--figures", "-l", "42", "--chunk-bytes", "4096",
                            "--reads-per-batch", "37", str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-300:]
        ctxs = [json.loads(line) for line in r.stderr.decode().splitlines() if line.startswith("{")]
        print(devices, ctxs)
        assert len(ctxs) == devices.count(",") + 1
        assert sum(c["recordsJudged"] for c in ctxs) == with_seq and sum(c["bytesReceived"] for c in ctxs) == len(text)
        assert all(c["recordsJudged"] > 0 for c in ctxs), ctxs
        chunks = [c["chunks"] for c in ctxs]
        assert max(chunks) - min(chunks) <= 1, chunks
        if len(ctxs) == 1:
            assert ctxs[0]["msCommit"] == 0.0 and ctxs[0]["msCarryWait"] == 0.0, ctxs
            assert chunks == [PARENT_CHUNKS]


def test_plain_gzip_inflated_on_the_device(dcli, tmp_path, monkeypatch):
    """TS_GZIP_DEVICE=1 (with TS_GZIP_MIN_BYTES=0 and small spans, so that a small file takes that source): the plain-gzipped
    text is decoded on the device by the feed, and the route answers what it answers for the plain file; a bad input likewise."""
    monkeypatch.setenv("TS_GZIP_DEVICE", "1")
    monkeypatch.setenv("TS_GZIP_MIN_BYTES", "0")
    monkeypatch.setenv("TS_GZIP_SPAN", "4096")
    flags = "-l 42"
    good = S.generated(31, 200, 30, 1500, header=LONG_HEADER)
    bad = S.generated(32, 100, 30, 900) + S.sam_line(b"l", b"ACGT", b"III") + S.generated(33, 20, header=b"")
    entries, want = {}, {}
    for tag, text in (("good", good), ("bad", bad)):
        p = tmp_path / (tag + ".sam.gz")
        p.write_bytes(gzip.compress(text, 6))
        entries[tag], want[tag] = str(p), expected(text, flags)
    assert want["good"][0] == "ok" and want["bad"][0] == "err"
    for chunk in CHUNKS:
        got = run_each(dcli, tmp_path, list(entries.values()), ["--device"] + flags.split() + ["--chunk-bytes", str(chunk)])
        for tag, entry in entries.items():
            assert got[entry] == want[tag], (tag, chunk, got[entry][0], got[entry][2])
