"""Assembly record filters on the two device routes (scanFastaToFilesDevice and annotateGfaDevice with a selector) through
tests/cpp/assembly_device_cli.cpp: --device against --host of the same binary on the same input with the same filters — the
same exit status, the same stdout (apart from the GFA line's three time fields), byte-equal stderr ("Sequence filter: ...",
library_bases, warnings, the refusal) and byte-equal output files.  The two checks underneath are compared with plain references
in tests/test_gpu_filter_check.py.  Every process is one bounded step."""
import glob
import gzip
import os
import random
import subprocess

import pytest

from tests import filtercheck as FC
from tests import harness as H
from tests.test_bam_subset import bgzf_fancy
from tests.test_fasta_chunk_reference_cpu import build_cli as build_fasta_cli
from tests.test_gfa_chunk_reference_cpu import build_cli as build_gfa_cli

pytestmark = pytest.mark.gpu

MULTI = H.golden_path("testFiles/multi.fa")                  # contig_t2t, contig_none, contig_incomplete
GAPPED = sorted(glob.glob(H.golden_path("testFiles/gapped_*.fa")))       # one record each: chr_gapped_<name>
GZ_FASTA = H.golden_path("testFiles/bTaeGut7_chr33_mat.fa.gz")
PATH_GFA = H.golden_path("testFiles/gfa_path_orient_pairs_small.gfa")    # path_pp, path_nn
PATHLESS_GFA = H.golden_path("testFiles/gfa_pathless_small.gfa")         # seg_t2t, seg_p, seg_q, seg_none
SHARED_GFA = H.golden_path("testFiles/gfa_single_seg_paths_small.gfa")   # path_plus, path_minus
FASTA_FLAGS = ["-w", "1000", "-s", "500", "-r", "-g", "-e", "-i"]
GFA_FLAGS = ["-x", "0", "-l", "60"]
ENCODINGS = ["plain", "bgzip", "gzip", "crlf"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return FC.build_driver(tmp_path_factory.mktemp("cpp") / "assembly_device_cli")


def files_of(d):
    return {os.path.relpath(p, str(d)): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(str(d), "**", "*"), recursive=True))
            if os.path.isfile(p)}


def run(cli, cwd, args, timeout=120):
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([cli] + [str(a) for a in args], cwd=str(cwd), stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout)


def comparable(stdout, gfa):
    """FASTA: the console text as it is.  GFA: the stats line without its parse, scan and write milliseconds."""
    return [line.split()[:-3] for line in stdout.split(b"\n") if line] if gfa else stdout


def both(driver, tmp_path, tag, path, args, device_args=(), gfa=False):
    """The device run and the host run of one command, each in a directory of its own with the same relative output directory:
    equal exit status, stdout, stderr and files; -> (device result, the device run's files)."""
    res, outs = [], []
    for route in ("--device", "--host"):
        cwd = tmp_path / (tag + route)
        res.append(run(driver, cwd, [route, path, "-o", "out"] + list(args) + (list(device_args) if route == "--device" else [])))
        outs.append(files_of(cwd / "out"))
    d, h = res
    assert d.returncode in (0, 1) and h.returncode in (0, 1), (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.returncode == h.returncode, (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.stderr == h.stderr, (d.stderr[-300:], h.stderr[-300:])
    assert comparable(d.stdout, gfa) == comparable(h.stdout, gfa)
    assert sorted(outs[0]) == sorted(outs[1])
    for name in outs[1]:
        assert outs[0][name] == outs[1][name], name
    return d, outs[0]


def encoded(tmp_path, stem, suffix, text, encoding, bom=False):
    """The text as a file of the given encoding; compressed files are named <stem><suffix>.gz."""
    data = {"plain": text, "bgzip": None, "gzip": None, "crlf": (b"\xef\xbb\xbf" if bom else b"") + text.replace(b"\n", b"\r\n")}[encoding]
    if encoding == "bgzip":
        data = bgzf_fancy(text, 1777, random.Random(5))
    elif encoding == "gzip":
        data = gzip.compress(text, 6)
    d = tmp_path / ("in_" + encoding)
    d.mkdir(exist_ok=True)
    p = d / (stem + suffix + (".gz" if encoding in ("bgzip", "gzip") else ""))
    p.write_bytes(data)
    return p


def ids_file(tmp_path, name, rows):
    p = tmp_path / name
    p.write_text("".join(r + "\n" for r in rows))
    return str(p)


# ------------------------------------------------------------------------------------------------------------ FASTA
def assembly_text():
    """multi.fa and the eight gapped fixtures as one assembly of eleven records."""
    texts = [open(p, "rb").read() for p in [MULTI] + GAPPED]
    return b"".join(t if t.endswith(b"\n") else t + b"\n" for t in texts)


def fasta_filters(tmp_path):
    return {
        "include": (["--include-prefix", "contig_t2t,chr_gapped_in"], 3),
        "exclude": (["--exclude-prefix", "chr_gapped_mis", "--exclude-bed", ids_file(tmp_path, "x.ids", ["contig_none"])], 8),
        "both": (["--include-prefix", "chr_", "--exclude-prefix", "chr_gapped_discordant"], 6),
        "bed_and_prefix": (["--include-bed", ids_file(tmp_path, "i.bed", ["chr_gapped_t2t\t0\t10", "contig_incomplete"]),
                            "--include-prefix", "chr_gapped_none", "--exclude-prefix", "contig_inc"], 2),
    }


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("which", ["include", "exclude", "both", "bed_and_prefix"])
def test_fasta_selection_equals_the_host_route(driver, tmp_path, which, encoding):
    """Eleven records, four selections, four encodings (CRLF with a byte order mark), a chunk that holds everything and one of
    4 KB that records cross; -m with one of the selections."""
    assert len(GAPPED) == 8
    filters, kept = fasta_filters(tmp_path)[which]
    path = encoded(tmp_path, "assembly", ".fa", assembly_text(), encoding, bom=True)
    flags = FASTA_FLAGS + (["-m"] if which == "both" else []) + ["--times"]
    for chunk in (None, 4096):
        d, files = both(driver, tmp_path, "c%s" % chunk, path, flags + filters, ["--chunk-bytes", chunk] if chunk else [])
        assert d.returncode == 0, d.stderr[-300:]
        assert b"Sequence filter: selected %d of 11 paths.\n" % kept in d.stderr and b"library_bases " in d.stderr
        assert len(files) >= 6 and any(v for v in files.values())
        report = [v for f, v in files.items() if f.endswith("_report.tsv")]
        assert report and report[0].count(b"\n") >= kept


def test_fasta_gzip_fixture_with_a_record_larger_than_the_chunk(driver, tmp_path):
    """The committed gzip assembly (one record of 4 MB): through the default chunk, and through chunks of 64 KB, which the one
    record makes grow."""
    for chunk in (None, 65536):
        d, files = both(driver, tmp_path, "c%s" % chunk, GZ_FASTA, ["--include-prefix", "chr33_mat", "--times"],
                        ["--chunk-bytes", chunk] if chunk else [])
        assert d.returncode == 0 and d.stderr.startswith(b"Sequence filter: selected 1 of 1 paths.\n"), d.stderr[-300:]


def test_fasta_without_filters_is_the_unfiltered_device_route(driver, tmp_path):
    """No filter option: the outputs of the existing entry point (tests/cpp/fasta_device_cli.cpp --device)."""
    old = build_fasta_cli(tmp_path / "fasta_device_cli")
    path = encoded(tmp_path, "assembly", ".fa", assembly_text(), "plain")
    new = run(driver, tmp_path / "new", ["--device", path, "-o", "out", "--chunk-bytes", 8192] + FASTA_FLAGS)
    ref = run(old, tmp_path / "old", ["--device", "--chunk-bytes", 8192, "-o", "out"] + FASTA_FLAGS + [path])
    assert new.returncode == ref.returncode == 0, (new.stderr[-300:], ref.stderr[-300:])
    assert new.stdout == ref.stdout and new.stderr == ref.stderr == b""
    assert files_of(tmp_path / "new" / "out") == files_of(tmp_path / "old" / "out") != {}


# ------------------------------------------------------------------------------------------------------------ GFA
def gfa_filters(tmp_path, gfa):
    a, b = {PATH_GFA: ("path_pp", "path_nn"), SHARED_GFA: ("path_plus", "path_minus"), PATHLESS_GFA: ("seg_t2t", "seg_q")}[gfa]
    return [["--include-prefix", a], ["--exclude-prefix", b], ["--include-prefix", a[:4], "--exclude-prefix", a],
            ["--include-bed", ids_file(tmp_path, "i.bed", [a + "\t0\t5"]), "--include-prefix", b]]


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("gfa", [PATH_GFA, PATHLESS_GFA, SHARED_GFA], ids=["paths", "pathless", "shared"])
def test_gfa_selection_equals_the_host_route(driver, tmp_path, gfa, encoding):
    """The three fixtures of tests/test_record_filters.py, include only, exclude only, both and BED plus prefix, four encodings,
    a chunk that holds everything and one of 64 bytes that every line crosses."""
    path = encoded(tmp_path, os.path.basename(gfa)[:-4], ".gfa", open(gfa, "rb").read(), encoding)
    nodes = set()
    for k, filters in enumerate(gfa_filters(tmp_path, gfa)):
        chunk = (None, 64)[k % 2] if encoding != "plain" else (64, None)[k % 2]
        d, files = both(driver, tmp_path, "f%d" % k, path, GFA_FLAGS + filters, ["--chunk-bytes", chunk] if chunk else [], gfa=True)
        assert d.returncode == 0 and b"Sequence filter: selected " in d.stderr, d.stderr[-300:]
        assert len(files) == 2
        nodes |= {l for v in files.values() for l in v.split(b"\n") if l.startswith(b"S\ttelomere_")}
    assert nodes


def test_gfa_without_filters_is_the_unfiltered_device_route(driver, tmp_path):
    old = build_gfa_cli(tmp_path / "gfa_device_cli")
    for k, gfa in enumerate((PATH_GFA, PATHLESS_GFA, H.golden_path("testFiles/gfa2_small.gfa"))):
        new = run(driver, tmp_path / ("new%d" % k), ["--device", gfa, "-o", "out", "--chunk-bytes", 256] + GFA_FLAGS)
        ref = run(old, tmp_path / ("old%d" % k), ["--device", "--chunk-bytes", 256, "-o", "out", "-f", gfa] + GFA_FLAGS)
        assert new.returncode == ref.returncode == 0, (new.stderr[-300:], ref.stderr[-300:])
        assert comparable(new.stdout, True) == comparable(ref.stdout, True) and new.stderr == ref.stderr
        assert files_of(tmp_path / ("new%d" % k) / "out") == files_of(tmp_path / ("old%d" % k) / "out") != {}


# ------------------------------------------------------------------------------------------------------------ refusals
def fa(records):
    return "".join(">%s\n%s\n" % (h, s) for h, s in records).encode()


MANY = "".join("zz%02d\n" % i for i in range(12)) + "contig_none\n"
# (file name, text or None for multi.fa / the pathless fixture, filters with %IDS% for a selector file of `ids`, ids, message):
# tests/test_record_filters.py's test_fasta_loader_errors, test_unmatched_and_excluding_everything, GFA_REJECTIONS and
# test_gfa_name_errors
REFUSALS = [
    ("dup.fa", fa([("a x", "ACGT"), ("b", "ACGT"), ("a\ty", "ACGT")]), ["--include-prefix", "a"], None,
     "Input contains duplicate primary sequence ID: 'a'."),
    ("noseq.fa", b">a\n>b\nACGT\n", ["--exclude-prefix", "b"], None, "FASTA record 'a' has no sequence."),
    ("last.fa", b">a\nACGT\n>b\n\n", ["--include-prefix", "a"], None, "FASTA record 'b' has no sequence."),
    ("eid.fa", b">a\nACGT\n> b\nACGT\n", ["--include-prefix", "a"], None, "FASTA input contains an empty primary sequence ID."),
    ("reads.fq", b"@r1\nACGT\n+\nIIII\n", ["--include-prefix", "r"], None, FC.NOT_FASTA),
    ("blank.fa", b"\n>a\nACGT\n", ["--include-prefix", "a"], None, FC.NOT_FASTA),
    ("empty.fa", b"", ["--include-prefix", "a"], None, "Assembly input is empty."),
    ("multi.fa", None, ["--include-bed", "%IDS%"], MANY,
     "Sequence filter ID(s) matched no input paths: " + ", ".join("'zz%02d'" % i for i in range(10)) + " (and 2 more)."),
    ("multi.fa", None, ["--include-prefix", "contig", "--exclude-prefix", "q,p"], None,
     "Sequence filter prefix(es) matched no input paths: 'p', 'q'."),
    ("multi.fa", None, ["--exclude-prefix", "contig_"], None, "Sequence filters excluded all input paths."),
    ("multi.fa", None, ["--include-prefix", "contig_t", "--exclude-prefix", "contig_t2t"], None, "Sequence filters excluded all input paths."),
    ("g.gfa2", b"H\tVN:Z:1.0\nS\ta\tACGT\n", ["--include-prefix", "a"], None, "Assembly record filters do not support GFA2" + FC.GFA2),
    ("g.GFA2.gz", b"S\ta\tACGT\n", ["--include-prefix", "a"], None, "Assembly record filters do not support GFA2" + FC.GFA2),
    ("g.gfa", b"# c\nH\tVN:Z:2.0\nS\ta\t4\tACGT\n", ["--include-prefix", "a"], None, "Assembly record filters do not support GFA2 at line 2" + FC.GFA2),
    ("g.gfa", b"H\tVN:Z:1.0\nS\ta\tACGT\nO\to1\ta+\n", ["--include-prefix", "a"], None,
     "Assembly record filters do not support GFA2 record type 'O' at line 3" + FC.GFA2),
    ("g.gfa", b"H\tVN:Z:1.1\nS\ta\tACGT\nW\tsm\t0\tc\t0\t4\t>a\n", ["--include-prefix", "a"], None,
     "Assembly record filters do not support GFA1 W walks at line 3" + FC.GFA2),
    ("g.gfa", b"S\ta\tACGT\nS\tb\tAC\nC\ta\t+\tb\t+\t0\t2M\n", ["--include-prefix", "a"], None,
     "Assembly record filters do not support GFA1 C containment records at line 3."),
    ("g.gfa", b"S\ta\t4\tACGT\n", ["--include-prefix", "a"], None, "Assembly record filters do not support GFA2 segment records at line 1" + FC.GFA2),
    ("g.gfa", b"S\ta\tACGT\nX\tfoo\n", ["--include-prefix", "a"], None, "Assembly record filters do not support GFA record type 'X' at line 2."),
    ("g.gfa", b"S\ta\tACGT\nSx\tb\n", ["--include-prefix", "a"], None, "Assembly record filters found a malformed or unsupported GFA record at line 2."),
    ("dup.gfa", b"S\ta\tACGT\nP\tp\ta+\t*\nP\tq\ta-\t*\nP\tp\ta-\t*\n", ["--include-prefix", "p"], None,
     "Input contains duplicate primary sequence ID(s): 'p'."),
    ("empty.gfa", b"S\ta\tACGT\nP\t\ta+\t*\n", ["--include-prefix", "a"], None, "Input contains an empty primary sequence ID."),
    ("pathless.gfa", None, ["--include-bed", "%IDS%"], "path_x\n", "Sequence filter ID(s) matched no input segments: 'path_x'."),
    ("pathless.gfa", None, ["--exclude-prefix", "seg_"], None, "Sequence filters excluded all input segments."),
    # two different offences in one input: the one the host route reports
    ("two.gfa", b"S\ta\tACGT\n# c\n\nW\tw\t0\tc\t0\t4\t>a\nS\tb\tAC\nO\to1\ta+\nS\tc\t4\tAC\n", ["--include-prefix", "a"], None,
     "Assembly record filters do not support GFA1 W walks at line 4" + FC.GFA2),
    ("two_cr.gfa", b"S\ta\tAC\rGT\r\nS\r\tb\tAC\r\nX\r\tq\r\nS\tc\t4\tAC\r\nO\tx\r\n", ["--include-prefix", "a"], None,
     "Assembly record filters do not support GFA record type 'X' at line 3."),
    ("two_and_twice.gfa", b"S\ta\tACGT\nS\ta\tAC\nC\ta\t+\ta\t+\t0\t2M\n", ["--include-prefix", "a"], None,
     "Assembly record filters do not support GFA1 C containment records at line 3."),
    ("two.fa", b">a\nAC\n>b\n\r\n>a\nGT\n>\nAC\n", ["--include-prefix", "a"], None, "FASTA record 'b' has no sequence."),
    ("two_dup_first.fa", b">a\nAC\n>a\nGT\n>c\n\n>d\nAC\n", ["--include-prefix", "a"], None, "Input contains duplicate primary sequence ID: 'a'."),
    ("front_and_dup.fa", b"x\n>a\nAC\n>a\nGT\n", ["--include-prefix", "a"], None, FC.NOT_FASTA),
    ("bom.gfa", b"\xef\xbb\xbfH\tVN:Z:1.0\nS\ta\tACGT\n", ["--include-prefix", "a"], None,
     "Assembly record filters found a malformed or unsupported GFA record at line 1."),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusals_are_the_host_routes(driver, tmp_path, k):
    """The same message and the same exit status on both routes, at a chunk that holds the input and at one of 64 bytes, nothing
    on stdout and an empty output directory."""
    name, text, filters, ids, message = REFUSALS[k]
    if text is None:
        text = open(MULTI if name == "multi.fa" else PATHLESS_GFA, "rb").read()
    d = tmp_path / "in"
    d.mkdir()
    path = d / name
    path.write_bytes(gzip.compress(text) if name.endswith(".gz") else text)
    if ids is not None:
        filters = [ids_file(tmp_path, "sel.ids", [ids.rstrip("\n")]) if f == "%IDS%" else f for f in filters]
    assert (FC.ref_gfa_offence(text) if name.endswith(".gfa") else FC.ref_fasta_offence(text) if name.endswith((".fa", ".fq")) else None) in (None, message)
    for chunk in (None, 64):
        res, files = both(driver, tmp_path, "c%s" % chunk, path, filters, ["--chunk-bytes", chunk] if chunk else [])
        assert res.returncode == 1 and res.stdout == b"" and not files
        assert res.stderr.decode().endswith("Error: %s\n" % message), res.stderr[-300:]


def test_resident_limit_refuses_and_names_the_host_route(driver, tmp_path):
    path = encoded(tmp_path, "assembly", ".fa", assembly_text(), "plain")
    size = os.path.getsize(str(path))
    r = run(driver, tmp_path / "limited", ["--device", path, "-o", "out", "--include-prefix", "contig_t2t", "--chunk-bytes", 4096,
                                           "--resident-limit", size // 2])
    assert r.returncode == 1 and r.stdout == b"" and not files_of(tmp_path / "limited" / "out")
    assert b"scanFastaToFiles, the host route" in r.stderr and b"does not fit" in r.stderr, r.stderr[-300:]
    r = run(driver, tmp_path / "roomy", ["--device", path, "-o", "out", "--include-prefix", "contig_t2t", "--chunk-bytes", 4096,
                                         "--resident-limit", 4 * size])
    assert r.returncode == 0 and r.stderr == b"Sequence filter: selected 1 of 11 paths.\n", r.stderr[-300:]
