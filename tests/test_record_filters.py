"""Assembly record filters (--include-bed / --exclude-bed / --include-prefix / --exclude-prefix; reference src/main.cpp:103-147,
src/input.cpp:151-665) through tests/cpp/assembly_cli.cpp, without a device: selections through its --selection-only hook
(the selection is resolved, validated and printed, then the driver stops before any device call), GFA annotations through
--ends-file with the per-end lengths of the CPU oracle's tips-only blocks, and cli.parse_cli on the same option strings."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from teloscope_amd import cli as pycli
from tests import harness as H
from tests import seqgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = H.golden_path("testFiles/multi.fa")                  # contig_t2t, contig_none, contig_incomplete
PATH_GFA = H.golden_path("testFiles/gfa_path_orient_pairs_small.gfa")
PATHLESS_GFA = H.golden_path("testFiles/gfa_pathless_small.gfa")
SHARED_GFA = H.golden_path("testFiles/gfa_single_seg_paths_small.gfa")
GZ_FASTA = H.golden_path("testFiles/bTaeGut7_chr33_mat.fa.gz")
GFA_FLAGS = ["-x", "0", "-l", "60"]                           # the flags of the fixtures' manifests (validateFiles/gfa_*.tst)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / "assembly_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "assembly_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def run(cli, *args):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def selected(cli, path, *filters):
    """(input index, ID) of every selected record, and the stderr line"""
    r = run(cli, path, "--selection-only", *filters)
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in r.stdout.splitlines()]
    return [(int(f[0]), f[1]) for f in rows], r.stderr


def refused(cli, tmp_path, args, message):
    """the run fails with `Error: <message>`, prints nothing on stdout and makes no output file"""
    out = tmp_path / "out_refused"
    r = run(cli, *args, "-o", out)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.endswith("Error: %s\n" % message), r.stderr
    assert r.stdout == ""
    assert not out.exists() or not list(out.iterdir())
    return r


def write(path, text, mode="w"):
    with open(path, mode) as fh:
        fh.write(text)
    return str(path)


def fasta(path, records):
    return write(path, "".join(">%s\n%s\n" % (h, s) for h, s in records))


# ------------------------------------------------------------------------------------------------------------ selection
def test_union_repetition_and_exclusion_precedence(cli, tmp_path):
    ids = write(tmp_path / "inc.ids", "contig_incomplete\n")
    got, err = selected(cli, MULTI, "--include-prefix", "contig_t2t", "--include-bed", ids, "--exclude-prefix", "contig_t2t")
    assert got == [(2, "contig_incomplete")]
    assert err == "Sequence filter: selected 1 of 3 paths.\n"
    got, _ = selected(cli, MULTI, "--include-prefix", "contig_t2t", "--include-bed", ids)
    assert got == [(0, "contig_t2t"), (2, "contig_incomplete")]
    got, err = selected(cli, MULTI, "--include-prefix", "contig_t2t", "--include-prefix", "contig_t2t,contig_t2t",
                        "--include-bed", ids, "--include-bed", ids)
    assert got == [(0, "contig_t2t"), (2, "contig_incomplete")] and "selected 2 of 3 paths." in err


def test_exclude_only(cli, tmp_path):
    got, err = selected(cli, MULTI, "--exclude-prefix", "contig_none")
    assert got == [(0, "contig_t2t"), (2, "contig_incomplete")] and err == "Sequence filter: selected 2 of 3 paths.\n"
    got, _ = selected(cli, MULTI, "--exclude-bed", write(tmp_path / "x.bed", "contig_t2t\t0\t5\n"))
    assert got == [(1, "contig_none"), (2, "contig_incomplete")]


def test_no_filter_selects_everything_silently(cli):
    got, err = selected(cli, MULTI)
    assert got == [(0, "contig_t2t"), (1, "contig_none"), (2, "contig_incomplete")] and err == ""


def test_prefixes_are_trimmed_literal_and_case_sensitive(cli, tmp_path):
    f = fasta(tmp_path / "p.fa", [("CM.1", "ACGT"), ("CMX1", "ACGT"), ("star*a", "ACGT"), ("stara", "ACGT"),
                                  ("Chr1", "ACGT"), ("chr1", "ACGT")])
    assert selected(cli, f, "--include-prefix", " CM. \t")[0] == [(0, "CM.1")]
    assert selected(cli, f, "--include-prefix", "star*")[0] == [(2, "star*a")]
    assert selected(cli, f, "--include-prefix", "chr")[0] == [(5, "chr1")]
    assert selected(cli, f, "--include-prefix", "Chr, CM.", "--exclude-prefix", "CM.1")[0] == [(4, "Chr1")]
    refused(cli, tmp_path, [f, "--include-prefix", "cm."], "Sequence filter prefix(es) matched no input paths: 'cm.'.")


def test_selector_file_with_bom_crlf_comments_and_bed_rows(cli, tmp_path):
    sel = tmp_path / "sel.bed"
    sel.write_bytes(b"\xef\xbb\xbftrack name=x\r\nbrowser position chr1\r\n# a comment\r\n\r\n"
                    b"contig_t2t\t0\t10\tname\t0\t+\r\ncontig_t2t\r\n  contig_incomplete \t 5 7 \r\n")
    got, err = selected(cli, MULTI, "--include-bed", sel)
    assert got == [(0, "contig_t2t"), (2, "contig_incomplete")] and "selected 2 of 3 paths." in err


@pytest.mark.parametrize("row", ["contig_t2t\t-1\t5", "contig_t2t\t+1\t5", "contig_t2t\t1a\t5", "contig_t2t\t10\t5",
                                 "contig_t2t\t0\t99999999999999999999"])
def test_selector_file_bad_coordinates(cli, tmp_path, row):
    sel = write(tmp_path / "bad.bed", "# header\n%s\n" % row)
    refused(cli, tmp_path, [MULTI, "--include-bed", sel],
            "%s:2 has invalid BED start/end coordinates." % os.path.realpath(sel))


def test_selector_file_two_columns_and_no_ids(cli, tmp_path):
    two = write(tmp_path / "two.bed", "contig_t2t\ncontig_none 5\n")
    refused(cli, tmp_path, [MULTI, "--exclude-bed", two],
            "%s:2 must contain either one ID column or at least three BED columns." % os.path.realpath(two))
    empty = write(tmp_path / "empty.ids", "# nothing\ntrack x\n\n")
    refused(cli, tmp_path, [MULTI, "--include-bed", empty],
            "--include-bed file '%s' contains no sequence IDs." % os.path.realpath(empty))


# ------------------------------------------------------------------------------------------------------------ option errors
OPTION_ERRORS = [
    (["--include-bed", "/nonexistent/ids.txt"], "--include-bed file does not exist: '/nonexistent/ids.txt'."),
    (["--exclude-bed", "/"], "--exclude-bed file '/' is not a regular file."),
    (["--include-prefix", ""], "--include-prefix contains an empty prefix."),
    (["--include-prefix", "a,"], "--include-prefix contains an empty prefix."),
    (["--exclude-prefix", "a,,b"], "--exclude-prefix contains an empty prefix."),
    (["--exclude-prefix", " , "], "--exclude-prefix contains an empty prefix."),
    (["--include-prefix=contig_t2t,"], "--include-prefix contains an empty prefix."),
    (["--fastq-subset", "--include-prefix", "contig"],
     "--include-bed/--exclude-bed/--include-prefix/--exclude-prefix filter assembly records and cannot be used in read subset mode."),
    (["--exclude-prefix", "contig", "--bam-subset"],
     "--include-bed/--exclude-bed/--include-prefix/--exclude-prefix filter assembly records and cannot be used in read subset mode."),
] + [([o], "Option %s is missing a required argument" % o)
     for o in ("--include-bed", "--exclude-bed", "--include-prefix", "--exclude-prefix")]


@pytest.mark.parametrize("args,message", OPTION_ERRORS, ids=[str(i) for i in range(len(OPTION_ERRORS))])
def test_option_errors_in_driver_and_parse_cli(cli, tmp_path, args, message):
    out = tmp_path / "out"
    r = run(cli, MULTI, "-o", out, *args)                      # (missing-argument cases: the option is the last word)
    assert r.returncode == 1 and r.stdout == "" and r.stderr == "Error: %s\n" % message, r.stderr
    assert not out.exists()
    with pytest.raises(pycli.SequenceFilterError) as e:
        pycli.parse_cli(" ".join([MULTI, "-o", str(out)] + ["'%s'" % a for a in args]))
    assert str(e.value) == message


def test_parse_cli_filter_fields(tmp_path):
    ids = write(tmp_path / "a.ids", "contig_t2t\n")
    o = pycli.parse_cli("%s -r -u --include-bed %s --exclude-bed=%s --include-prefix ' hap1_, hap2_' "
                        "--include-prefix hap1_ --exclude-prefix=unplaced -o out" % (MULTI, ids, ids))
    assert o.input == MULTI and o.out_win_repeats and not o.ultra_fast
    assert o.include_bed_files == [os.path.realpath(ids)] and o.exclude_bed_files == [os.path.realpath(ids)]
    assert o.include_prefixes == ["hap1_", "hap2_", "hap1_"] and o.exclude_prefixes == ["unplaced"]
    assert o.sequence_filter_active
    plain = pycli.parse_cli("%s -r -w 500 -s 250" % MULTI)
    assert not plain.sequence_filter_active and plain.include_prefixes == [] and plain.window_size == 500


# ------------------------------------------------------------------------------------------------------------ FASTA input
def test_primary_id_is_cut_at_whitespace(cli, tmp_path):
    f = fasta(tmp_path / "d.fa", [("contig_a\tdescription here", "ACGTN"), ("contig_b more", "ACGT"),
                                  ("contig_c\x0bvt", "AC")])
    got, err = selected(cli, f, "--include-prefix", "contig_")
    assert got == [(0, "contig_a"), (1, "contig_b"), (2, "contig_c")] and "selected 3 of 3 paths." in err
    assert selected(cli, f, "--include-bed", write(tmp_path / "i", "contig_a\n"))[0] == [(0, "contig_a")]


def test_fasta_loader_errors(cli, tmp_path):
    dup = fasta(tmp_path / "dup.fa", [("a x", "ACGT"), ("b", "ACGT"), ("a\ty", "ACGT")])
    refused(cli, tmp_path, [dup, "--include-prefix", "a"], "Input contains duplicate primary sequence ID: 'a'.")
    noseq = write(tmp_path / "noseq.fa", ">a\n>b\nACGT\n")
    refused(cli, tmp_path, [noseq, "--exclude-prefix", "b"], "FASTA record 'a' has no sequence.")
    lastempty = write(tmp_path / "last.fa", ">a\nACGT\n>b\n\n")
    refused(cli, tmp_path, [lastempty, "--include-prefix", "a"], "FASTA record 'b' has no sequence.")
    emptyid = write(tmp_path / "eid.fa", ">a\nACGT\n> b\nACGT\n")
    refused(cli, tmp_path, [emptyid, "--include-prefix", "a"], "FASTA input contains an empty primary sequence ID.")
    fq = write(tmp_path / "reads.fq", "@r1\nACGT\n+\nIIII\n")
    refused(cli, tmp_path, [fq, "--include-prefix", "r"], "Assembly record filters require FASTA input or a recognized GFA file.")
    blank = write(tmp_path / "blank.fa", "\n>a\nACGT\n")
    refused(cli, tmp_path, [blank, "--include-prefix", "a"], "Assembly record filters require FASTA input or a recognized GFA file.")
    empty = write(tmp_path / "empty.fa", "")
    refused(cli, tmp_path, [empty, "--include-prefix", "a"], "Assembly input is empty.")


def test_unmatched_and_excluding_everything(cli, tmp_path):
    many = write(tmp_path / "many.ids", "".join("zz%02d\n" % i for i in range(12)) + "contig_none\n")
    refused(cli, tmp_path, [MULTI, "--include-bed", many],
            "Sequence filter ID(s) matched no input paths: " + ", ".join("'zz%02d'" % i for i in range(10)) + " (and 2 more).")
    refused(cli, tmp_path, [MULTI, "--include-prefix", "contig", "--exclude-prefix", "q,p"],
            "Sequence filter prefix(es) matched no input paths: 'p', 'q'.")
    refused(cli, tmp_path, [MULTI, "--exclude-prefix", "contig_"], "Sequence filters excluded all input paths.")
    refused(cli, tmp_path, [MULTI, "--include-prefix", "contig_t", "--exclude-prefix", "contig_t2t"],
            "Sequence filters excluded all input paths.")


def test_bom_crlf_and_gzip_fasta(cli, tmp_path):
    with open(MULTI, "rb") as fh:
        text = fh.read()
    bom = tmp_path / "bom.fa"
    bom.write_bytes(b"\xef\xbb\xbf" + text.replace(b"\n", b"\r\n"))
    gz = tmp_path / "multi.fa.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    want = selected(cli, MULTI, "--exclude-prefix", "contig_none")
    assert selected(cli, bom, "--exclude-prefix", "contig_none") == want
    assert selected(cli, gz, "--exclude-prefix", "contig_none") == want
    got, err = selected(cli, GZ_FASTA, "--include-prefix", "chr33_mat")
    assert got == [(0, "chr33_mat")] and err == "Sequence filter: selected 1 of 1 paths.\n"


def test_fasta_in_a_directory_named_like_gfa(cli, tmp_path):
    d = tmp_path / "x.gfa.archive"
    d.mkdir()
    shutil.copy(MULTI, d / "assembly.fa")
    r = run(cli, d / "assembly.fa", "--selection-only", "--include-prefix", "contig_none")
    assert r.returncode == 0 and r.stdout == "1\tcontig_none\t2000\t0\n", r.stderr


@pytest.mark.parametrize("join", [False, True], ids=["text_pieces", "joined"])
def test_group_reader_keeps_only_selected_records(cli, tmp_path, join):
    """a mapped file cut into many small groups: only kept records come out, in order, with their input indices and
    bases; a group holds at most group-bytes of kept text unless it is one record"""
    rng = np.random.default_rng(7)
    recs = []
    for i in range(40):
        seq = seqgen.chromosome(rng, int(rng.integers(500, 4000)), telo_repeats=20, n_its=0,
                                n_runs=int(i % 3 == 0)).decode()
        recs.append(("rec%02d" % i, seq))
    path = tmp_path / "many.fa"
    with open(path, "w") as fh:
        for h, s in recs:
            fh.write(">%s some words\n" % h + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    keep = [i for i in range(40) if i % 3 == 1 or i in (0, 39, 17)]
    ids = write(tmp_path / "keep.ids", "".join("rec%02d\n" % i for i in keep))
    args = [path, "--selection-only", "--include-bed", ids, "--group-bytes", 5000] + (["--join-lines"] if join else [])
    r = run(cli, *args)
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in r.stdout.splitlines()]
    assert [int(f[0]) for f in rows] == keep
    assert [f[1] for f in rows] == ["rec%02d" % i for i in keep]
    assert [int(f[2]) for f in rows] == [len(recs[i][1]) for i in keep]
    groups = {}
    for f in rows:
        groups.setdefault(int(f[3]), []).append(int(f[0]))
    assert len(groups) > 5
    for g in groups.values():
        text = sum(len(recs[i][1]) + (len(recs[i][1]) + 59) // 60 for i in g)
        assert len(g) == 1 or text <= 5000
    assert r.stderr == "Sequence filter: selected %d of 40 paths.\n" % len(keep)


# ------------------------------------------------------------------------------------------------------------ GFA input
GFA_REJECTIONS = [
    ("g.gfa2", "H\tVN:Z:1.0\nS\ta\tACGT\n", "Assembly record filters do not support GFA2; use GFA1 P paths or a pathless GFA1 graph."),
    ("g.GFA2.gz", None, "Assembly record filters do not support GFA2; use GFA1 P paths or a pathless GFA1 graph."),
    ("g.gfa", "# c\nH\tVN:Z:2.0\nS\ta\t4\tACGT\n",
     "Assembly record filters do not support GFA2 at line 2; use GFA1 P paths or a pathless GFA1 graph."),
    ("g.gfa", "H\tVN:Z:1.0\nS\ta\tACGT\nO\to1\ta+\n",
     "Assembly record filters do not support GFA2 record type 'O' at line 3; use GFA1 P paths or a pathless GFA1 graph."),
    ("g.gfa", "H\tVN:Z:1.1\nS\ta\tACGT\nW\tsm\t0\tc\t0\t4\t>a\n",
     "Assembly record filters do not support GFA1 W walks at line 3; use GFA1 P paths or a pathless GFA1 graph."),
    ("g.gfa", "S\ta\tACGT\nS\tb\tAC\nC\ta\t+\tb\t+\t0\t2M\n",
     "Assembly record filters do not support GFA1 C containment records at line 3."),
    ("g.gfa", "S\ta\t4\tACGT\n",
     "Assembly record filters do not support GFA2 segment records at line 1; use GFA1 P paths or a pathless GFA1 graph."),
    ("g.gfa", "S\ta\tACGT\nX\tfoo\n", "Assembly record filters do not support GFA record type 'X' at line 2."),
    ("g.gfa", "S\ta\tACGT\nSx\tb\n", "Assembly record filters found a malformed or unsupported GFA record at line 2."),
]


@pytest.mark.parametrize("name,text,message", GFA_REJECTIONS, ids=[str(i) for i in range(len(GFA_REJECTIONS))])
def test_gfa_rejections(cli, tmp_path, name, text, message):
    path = write(tmp_path / name, text or "S\ta\tACGT\n")
    refused(cli, tmp_path, [path, "--include-prefix", "a"], message)


def test_unfiltered_gfa_still_reads_what_it_read(cli, tmp_path):
    """without filters W lines pass and GFA 2 segments are read, as before"""
    w = write(tmp_path / "w.gfa", "H\tVN:Z:1.1\nS\ta\tACGT\nW\tsm\t0\tc\t0\t4\t>a\n")
    assert selected(cli, w)[0] == [(0, "a")]
    g2 = write(tmp_path / "g2.gfa", "H\tVN:Z:2.0\nS\ta\t4\tACGT\n")
    assert selected(cli, g2)[0] == [(0, "a")]


def test_gfa_name_errors(cli, tmp_path):
    dup = write(tmp_path / "dup.gfa", "S\ta\tACGT\nP\tp\ta+\t*\nP\tq\ta-\t*\nP\tp\ta-\t*\n")
    refused(cli, tmp_path, [dup, "--include-prefix", "p"], "Input contains duplicate primary sequence ID(s): 'p'.")
    empty = write(tmp_path / "empty.gfa", "S\ta\tACGT\nP\t\ta+\t*\n")
    refused(cli, tmp_path, [empty, "--include-prefix", "a"], "Input contains an empty primary sequence ID.")
    refused(cli, tmp_path, [PATHLESS_GFA, "--include-bed", write(tmp_path / "i", "path_x\n")],
            "Sequence filter ID(s) matched no input segments: 'path_x'.")
    refused(cli, tmp_path, [PATHLESS_GFA, "--exclude-prefix", "seg_"], "Sequence filters excluded all input segments.")


def oracle_ends(gfa, path):
    """per segment with a sequence: the longest of the CPU oracle's tips-only terminal blocks on either side"""
    from tests.backends import OracleBackend
    backend = OracleBackend(H.parse_cli(" ".join([gfa] + GFA_FLAGS)))
    segs, _ = H.parse_gfa(gfa)
    with open(path, "w") as fh:
        for name, seq in segs.items():
            if seq is None:
                continue
            best = [0, 0]
            for b in backend.scan_segment(seq.upper().encode(), 0, True)["terminal_blocks"]:
                start, ln = int(b["start"]), int(b["block_len"])
                side = 0 if start <= len(seq) - (start + ln) else 1
                best[side] = max(best[side], ln)
            fh.write("%s\t%d\t%d\n" % (name, best[0], best[1]))
    return str(path)


def annotated(cli, tmp_path, gfa, *filters, ends=None):
    out = tmp_path / "gfa_out"
    args = [gfa, "-o", out, "-j", "4"] + GFA_FLAGS + list(filters)
    if ends:
        args += ["--ends-file", ends]
    r = run(cli, *args)
    assert r.returncode == 0, r.stderr
    name = os.path.basename(gfa)
    with open(out / (name + ".telo.annotated.gfa")) as fh:
        lines = fh.read().split("\n")
    with open(out / (name + ".telo.annotated.colors.csv")) as fh:
        colors = fh.read().splitlines()
    nodes = [l.split("\t")[1] for l in lines if l.startswith("S\ttelomere_")]
    with open(gfa) as fh:
        src = fh.read().rstrip("\n").split("\n")
    assert lines[:len(src)] == src                                # every input line, unselected P lines included
    assert colors[0] == "node\tcolor" and [c.split("\t")[0] for c in colors[1:]] == nodes
    assert all(c.endswith("\t#008000") for c in colors[1:])
    shutil.rmtree(out)
    return sorted(nodes), r.stderr


GFA_SELECTIONS = [
    (SHARED_GFA, ["--include-prefix", "path_plus"], ["telomere_seg_shared+_end", "telomere_seg_shared+_start"],
     "selected 1 of 2 paths."),
    (SHARED_GFA, ["--exclude-prefix", "path_plus"], ["telomere_seg_shared-_end", "telomere_seg_shared-_start"],
     "selected 1 of 2 paths."),
    (PATH_GFA, ["--include-prefix", "path_nn"], None, "selected 1 of 2 paths."),
    (PATHLESS_GFA, ["--include-prefix", "seg_t2t,seg_q"], None, "selected 2 of 4 segments."),
]


@pytest.mark.parametrize("gfa,filters,nodes,line", GFA_SELECTIONS, ids=["shared_plus", "shared_minus", "paths", "pathless"])
def test_gfa_selection_host_replay(cli, tmp_path, gfa, filters, nodes, line):
    ends = oracle_ends(gfa, tmp_path / "ends.tsv")
    got, err = annotated(cli, tmp_path, gfa, *filters, ends=ends)
    assert "Sequence filter: " + line in err
    every, err0 = annotated(cli, tmp_path, gfa, ends=ends)
    assert "Sequence filter" not in err0
    if nodes is not None:
        assert got == nodes
    _, paths = H.parse_gfa(gfa)
    if paths:
        keep = [p for p, _ in paths if any(p.startswith(x) for x in filters[1].split(","))]
        if filters[0] == "--exclude-prefix":
            keep = [p for p, _ in paths if p not in keep]
        segs = {c[0] for p, comps in paths if p in keep for c in (comps[0], comps[-1])}
    else:
        segs = set(filters[1].split(","))
    assert got and set(got) <= set(every)
    assert {n[len("telomere_"):].rsplit("_", 1)[0][:-1] for n in got} <= segs
