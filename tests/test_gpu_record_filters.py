"""Assembly record filters on the device (tests/cpp/assembly_cli.cpp).  The oracle: a filtered run of a FASTA must write what
an unfiltered run of the same driver writes for a FASTA that holds only the selected records, in order — the eleven files
and the console path table byte for byte, except the `pos` column, which keeps each record's index in the whole input, and
the summary, which gains the two filter lines.  Plus the bases handed to the library, a gzip input, GFA selections against
the host replay, and byte identity with manifest_cli / gfa_cli when no filter is given."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import seqgen
from tests.test_record_filters import GFA_FLAGS, GZ_FASTA, MULTI, PATH_GFA, PATHLESS_GFA, SHARED_GFA, oracle_ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIXES = ["_window_repeat_density.bedgraph", "_window_canonical_ratio.bedgraph", "_window_strand_ratio.bedgraph",
            "_window_gc.bedgraph", "_window_entropy.bedgraph", "_canonical_matches.bed", "_noncanonical_matches.bed",
            "_terminal_telomeres.bed", "_interstitial_telomeres.bed", "_gaps.bed", "_report.tsv"]


def _build(tmp_path_factory, name):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / name
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return {n: _build(tmp_path_factory, n) for n in ("assembly_cli", "manifest_cli", "gfa_cli")}


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def split_report(text):
    """(table rows as field lists, the other lines) of a console / report text"""
    rows, rest = [], []
    for line in text.split("\n"):
        f = line.split("\t")
        if len(f) >= 2 and f[0].isdigit():
            rows.append(f)
        else:
            rest.append(line)
    return rows, rest


def records_of(path):
    """(header line, body text) per record, as written"""
    with open(path) as fh:
        text = fh.read()
    assert text.startswith(">")
    out = []
    for chunk in text[1:].split("\n>"):
        head, _, body = chunk.partition("\n")
        out.append((">" + head, body))
    return out


def assert_filtered_equals_subset(cli, tmp_path, src, flags, filters, extra=()):
    sel = run(cli, src, "--selection-only", *filters, *extra).stdout.splitlines()
    index = [int(l.split("\t")[0]) for l in sel]
    recs = records_of(src)
    sub_dir = tmp_path / "subset"
    sub_dir.mkdir()
    sub = sub_dir / os.path.basename(src)
    with open(sub, "w") as fh:
        for i in index:
            h, body = recs[i]
            fh.write(h + "\n" + body + ("" if body.endswith("\n") else "\n"))
    a, b = tmp_path / "filtered", tmp_path / "plain"
    ra = run(cli, src, "-o", a, *flags, *filters, *extra, "--times")
    rb = run(cli, sub, "-o", b, *flags, *extra, "--times")
    name = os.path.basename(src)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(a)
    for sfx in SUFFIXES:
        fa, fb = a / (name + sfx), b / (name + sfx)
        assert fa.exists() == fb.exists()
        if fa.exists() and sfx != "_report.tsv":
            assert read(fa) == read(fb), sfx
    nsel = "Sequence filter: selected %d of %d paths." % (len(index), len(recs))
    assert nsel in ra.stderr and "Sequence filter" not in rb.stderr
    for ta, tb in ((ra.stdout, rb.stdout), (read(a / (name + "_report.tsv")).decode(), read(b / (name + "_report.tsv")).decode())):
        rows_a, rest_a = split_report(ta)
        rows_b, rest_b = split_report(tb)
        assert [r[1:] for r in rows_a] == [r[1:] for r in rows_b]
        assert [int(r[0]) for r in rows_a] == [i + 1 for i in index]            # pos: the input index
        assert [int(r[0]) for r in rows_b] == list(range(1, len(index) + 1))
        at = rest_b.index("Total paths:\t%d" % len(index)) + 1
        assert rest_a == rest_b[:at] + ["Filter input paths:\t%d" % len(recs), "Filter selected paths:\t%d" % len(index)] + rest_b[at:]
    bases = lambda r: int(re.search(r"library_bases (\d+)", r.stderr).group(1))   # noqa: E731
    gaps = sum(len(re.findall(r"[NnXx]", recs[i][1])) for i in index)
    assert bases(ra) == bases(rb) == sum(len(recs[i][1].replace("\n", "").replace("\r", "")) for i in index) - gaps
    return index


@pytest.mark.gpu
@pytest.mark.parametrize("filters", [["--include-prefix", "contig_t2t,contig_incomplete"], ["--exclude-prefix", "contig_none"],
                                     ["--include-bed", "IDS"], ["--include-prefix", "contig_t2t", "--include-bed", "IDS",
                                                                "--exclude-prefix", "contig_t2t"]],
                         ids=["prefixes", "exclude", "bed", "precedence"])
def test_multi_fa_filtered_equals_subset(drivers, tmp_path, filters):
    ids = tmp_path / "sel.ids"
    ids.write_text("contig_incomplete\n")
    filters = [str(ids) if f == "IDS" else f for f in filters]
    assert_filtered_equals_subset(drivers["assembly_cli"], tmp_path, MULTI, ["-r", "-g", "-e", "-m", "-i"], filters)


@pytest.fixture(scope="module")
def scattered(tmp_path_factory):
    """about 40 records, some with N-runs, 60-column lines"""
    rng = np.random.default_rng(11)
    path = tmp_path_factory.mktemp("fa") / "scattered.fa"
    with open(path, "w") as fh:
        for i in range(41):
            s = seqgen.chromosome(rng, int(rng.integers(3_000, 60_000)), n_its=2, n_runs=2 if i % 4 == 0 else 0).decode()
            fh.write(">scaf_%02d desc %d\n" % (i, i) + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    return str(path)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--join-lines"]], ids=["text_pieces", "joined"])
def test_scattered_selection_across_groups(drivers, tmp_path, scattered, extra):
    keep = [i for i in range(41) if i % 5 in (1, 2) or i in (0, 40)]
    ids = tmp_path / "keep.bed"
    ids.write_text("".join("scaf_%02d\t0\t10\n" % i for i in keep))
    index = assert_filtered_equals_subset(drivers["assembly_cli"], tmp_path, scattered, ["-w", "500", "-s", "250", "-r", "-g", "-i"],
                                          ["--include-bed", ids], ["--group-bytes", 60_000] + extra)
    assert index == keep


@pytest.mark.gpu
def test_gzip_fasta_selection(drivers, tmp_path):
    r = run(drivers["assembly_cli"], GZ_FASTA, "-o", tmp_path, "--include-prefix", "chr33_mat", "-u")
    assert "Sequence filter: selected 1 of 1 paths." in r.stderr
    assert "Scaffold N50:\t4246341\n" in r.stdout and "Filter selected paths:\t1\n" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("gfa,filters", [(SHARED_GFA, ["--include-prefix", "path_plus"]), (PATH_GFA, ["--exclude-prefix", "path_pp"]),
                                         (PATHLESS_GFA, ["--include-prefix", "seg_t2t,seg_q"])], ids=["shared", "paths", "pathless"])
def test_gfa_selection_on_device(drivers, tmp_path, gfa, filters):
    cli = drivers["assembly_cli"]
    ends = oracle_ends(gfa, tmp_path / "ends.tsv")
    dev, host = tmp_path / "dev", tmp_path / "host"
    r = run(cli, gfa, "-o", dev, *GFA_FLAGS, *filters)
    assert "Sequence filter: selected 1 of 2 paths." in r.stderr or "selected 2 of 4 segments." in r.stderr
    run(cli, gfa, "-o", host, *GFA_FLAGS, *filters, "--ends-file", ends)
    stem = os.path.basename(gfa) + ".telo.annotated"
    for sfx in (".gfa", ".colors.csv"):
        assert read(dev / (stem + sfx)) == read(host / (stem + sfx))
    out = read(dev / (stem + ".gfa")).decode()
    assert "S\ttelomere_" in out
    if gfa == SHARED_GFA:
        assert sorted(re.findall(r"S\t(telomere_\S+)", out)) == ["telomere_seg_shared+_end", "telomere_seg_shared+_start"]


@pytest.mark.gpu
def test_no_filter_matches_manifest_cli_and_gfa_cli(drivers, tmp_path):
    a, m = tmp_path / "a", tmp_path / "m"
    m.mkdir()
    flags = ["-r", "-g", "-e", "-m", "-i"]
    ra = run(drivers["assembly_cli"], MULTI, "-o", a, *flags)
    rm = run(drivers["manifest_cli"], "-f", MULTI, *flags, "--out-base", m / "multi.fa")
    assert ra.stdout == rm.stdout and "Sequence filter" not in ra.stderr
    for sfx in SUFFIXES:
        assert read(a / ("multi.fa" + sfx)) == read(m / ("multi.fa" + sfx)), sfx
    ga, gg = tmp_path / "ga", tmp_path / "gg"
    gg.mkdir()
    run(drivers["assembly_cli"], PATH_GFA, "-o", ga, *GFA_FLAGS)
    run(drivers["gfa_cli"], "-f", PATH_GFA, "-o", gg, *GFA_FLAGS)
    stem = os.path.basename(PATH_GFA) + ".telo.annotated"
    for sfx in (".gfa", ".colors.csv"):
        assert read(ga / (stem + sfx)) == read(gg / (stem + sfx))
