"""GFA annotation mode (include/teloscope_mi355x_gfa.hpp) driven by tests/cpp/gfa_cli.cpp over the reference's 15 GFA
manifests (validateFiles/gfa*.tst): `teloscope asm.gfa -o out/` must write the annotated graph and its colours file that
the reference's validator accepts (src/validate.cpp:378-720, restated below).

  * on a GPU: the whole front end, per-end lengths from ts_terminal_ends;
  * on any machine: the same manifests with the per-end lengths taken from the CPU oracle's tips-only terminal blocks
    (the driver's --ends-file hook), so that parsing, end resolution and writing are checked without a device."""
import collections
import glob
import gzip
import os
import shlex
import shutil
import subprocess

import pytest

from tests import harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFA_MANIFESTS = sorted(glob.glob(os.path.join(H.GOLDEN, "validateFiles", "gfa*.tst")))
IDS = [os.path.basename(p) for p in GFA_MANIFESTS]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / "gfa_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gfa_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


# ---------------------------------------------------------------------------------------- the validator's GFA checks
def _tags(fields):
    tags = {}
    for f in fields:
        parts = f.split(":")
        if len(parts) >= 3 and len(parts[0]) >= 2:
            tags[parts[0]] = ":".join(parts[2:])
    return tags


def parse_doc(path):
    """parseGfa (src/validate.cpp:378-443): the header version, the telomere nodes and connectors, and the multisets of
    the other raw lines and of the other segments' keys."""
    doc = dict(version="", tel_segs=[], tel_conns=[], raw=collections.Counter(), seg_keys=collections.Counter())
    with open(path, "rb") as fh:
        lines = fh.read().decode().split("\n")
    for line in lines:
        line = line[:-1] if line.endswith("\r") else line
        if not line:
            continue
        f = line.split("\t")
        if f[0] == "H":
            for x in f[1:]:
                if x.startswith("VN:Z:"):
                    doc["version"] = x[5:]
            doc["raw"][line] += 1
        elif f[0] == "S" and len(f) >= 3:
            if doc["version"][:1] == "2" and len(f) >= 4:
                seq, tags = f[3], _tags(f[4:])
            else:
                seq, tags = f[2], _tags(f[3:])
            if f[1].startswith("telomere_"):
                doc["tel_segs"].append((f[1], tags))
            else:
                doc["raw"][line] += 1
                doc["seg_keys"][(f[1], seq, tuple(sorted(tags.items())))] += 1
        elif f[0] in ("L", "J") and len(f) >= 6:
            if f[1].startswith("telomere_") or f[3].startswith("telomere_"):
                doc["tel_conns"].append(dict(type=f[0], frm=f[1], fo=f[2][:1], to=f[3], to_o=f[4][:1], payload=f[5],
                                             tags=_tags(f[6:])))
            else:
                doc["raw"][line] += 1
        else:
            doc["raw"][line] += 1
    return doc


def read_expect(path):
    with open(path) as fh:
        rows = [l.rstrip("\r\n") for l in fh if l.strip() and not l.startswith("#")]
    head = rows[0].split("\t")
    return [dict(zip(head, r.split("\t"))) for r in rows[1:]]


def check_manifest(m, input_path, outdir, rc, stderr):
    d = collections.defaultdict(list)
    for k, v in m["directives"]:
        d[k].append(v)
    assert rc == int(d["expect_exit"][0]), stderr
    name = d["expect_output_name"][0]
    out_gfa = os.path.join(outdir, name)
    assert os.path.exists(out_gfa)
    out = parse_doc(out_gfa)
    if d.get("expect_gfa_header"):
        assert out["version"] == d["expect_gfa_header"][0]
    for rel in d.get("gfa_expect", []):
        rows = read_expect(H.golden_path(rel))
        assert sorted(n for n, _ in out["tel_segs"]) == sorted(r["node_name"] for r in rows)
        assert len(out["tel_conns"]) == len(rows)
        for r in rows:
            orient = r["path_orient"]
            assert r["node_name"] == "telomere_%s%s_%s" % (r["segment"], "+" if orient == "." else orient, r["terminal_role"])
            segs = [t for n, t in out["tel_segs"] if n == r["node_name"]]
            assert len(segs) == 1
            assert segs[0].get("LN") == "6" and segs[0].get("RC") == "6000" and segs[0].get("TL") == str(int(r["tl_bp"]))
            conns = [c for c in out["tel_conns"] if c["frm"] == r["node_name"]]
            assert len(conns) == 1
            c = conns[0]
            assert (c["type"], c["fo"], c["to"], c["to_o"], c["payload"]) == \
                (r["connector_type"], "+", r["segment"], r["seg_edge_orient"], r["connector_value"])
            assert c["tags"].get("RC") == "0"
    for mode in d.get("gfa_preserve_input", []):
        inp = parse_doc(input_path)
        if mode == "strict":
            assert inp["raw"] == out["raw"]
        elif mode == "subset":
            assert not (inp["raw"] - out["raw"])
        elif mode == "segments_only":
            assert inp["seg_keys"] == out["seg_keys"]
        else:
            raise AssertionError("unknown gfa_preserve_input mode " + mode)
    if d.get("expect_gfa_colors"):
        colors = os.path.join(outdir, name[:-len(".gfa")] + ".colors.csv")
        with open(colors) as fh:
            lines = [l.rstrip("\r\n") for l in fh if l.strip()]
        assert lines[0] == "node\tcolor"
        assert all(l.split("\t")[1] == "#008000" for l in lines[1:])
        assert sorted(l.split("\t")[0] for l in lines[1:]) == sorted(n for n, _ in out["tel_segs"])


def manifest_args(m, outdir):
    args = []
    for tok in shlex.split(m["command"]):
        if tok.startswith("testFiles/"):
            tok = H.golden_path(tok)
        args.append(outdir if tok == "%OUTDIR%" else tok)
    return args


def oracle_ends_file(m, path):
    """per segment with a sequence: the longest of the CPU oracle's tips-only terminal blocks on either side"""
    from tests.backends import OracleBackend
    opts = H.parse_cli(" ".join(t for t in m["command"].split() if t not in ("-o", "%OUTDIR%")))
    backend = OracleBackend(opts)
    segs, _ = H.parse_gfa(H.golden_path(opts.input))
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


# ---------------------------------------------------------------------------------------- tests
def test_fifteen_gfa_manifests():
    assert len(GFA_MANIFESTS) == 15


@pytest.mark.gpu
@pytest.mark.parametrize("path", GFA_MANIFESTS, ids=IDS)
def test_gfa_manifest_on_gpu(cli, tmp_path, path):
    m = H.load_manifest(path)
    args = manifest_args(m, str(tmp_path))
    r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=300)
    check_manifest(m, args[args.index("-f") + 1], str(tmp_path), r.returncode, r.stderr)
    if os.path.basename(path) == "gfa_noseq_small.tst":
        assert "2 of 2 GFA segment(s) had no sequence" in r.stderr


@pytest.mark.parametrize("path", GFA_MANIFESTS, ids=IDS)
def test_gfa_manifest_host_replay(cli, tmp_path, path):
    m = H.load_manifest(path)
    outdir = tmp_path / "out"
    outdir.mkdir()
    ends = str(tmp_path / "ends.tsv")
    oracle_ends_file(m, ends)
    args = manifest_args(m, str(outdir))
    r = subprocess.run([cli] + args + ["--ends-file", ends], capture_output=True, text=True, timeout=120)
    check_manifest(m, args[args.index("-f") + 1], str(outdir), r.returncode, r.stderr)
    if os.path.basename(path) == "gfa_noseq_small.tst":
        assert "2 of 2 GFA segment(s) had no sequence" in r.stderr


def test_gfa_gzip_input_host_replay(cli, tmp_path):
    """a .gfa.gz input is read through zlib; the output is named after the input file"""
    m = H.load_manifest(os.path.join(H.GOLDEN, "validateFiles", "gfa_path_orient_pairs_small.tst"))
    src = H.golden_path("testFiles/gfa_path_orient_pairs_small.gfa")
    gz = tmp_path / "graph.gfa.gz"
    with open(src, "rb") as fi, gzip.open(gz, "wb") as fo:
        shutil.copyfileobj(fi, fo)
    ends = str(tmp_path / "ends.tsv")
    oracle_ends_file(m, ends)
    r = subprocess.run([cli, "-f", str(gz), "-o", str(tmp_path), "--ends-file", ends], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain = tmp_path / "plain"
    plain.mkdir()
    r2 = subprocess.run([cli, "-f", src, "-o", str(plain), "--ends-file", ends], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    with open(tmp_path / "graph.gfa.gz.telo.annotated.gfa", "rb") as a, \
            open(plain / "gfa_path_orient_pairs_small.gfa.telo.annotated.gfa", "rb") as b:
        assert a.read() == b.read()


def test_gfa2_foreign_record_refused(cli, tmp_path):
    """GFA 2 records other than H and S are refused with a message and a nonzero exit status"""
    g = tmp_path / "edges.gfa"
    g.write_text("H\tVN:Z:2.0\nS\ta\t8\tACGTACGT\nS\tb\t8\tACGTACGT\nE\te1\ta+\tb+\t8\t8$\t0\t0\t0M\n")
    ends = tmp_path / "ends.tsv"
    ends.write_text("")
    r = subprocess.run([cli, "-f", str(g), "-o", str(tmp_path), "--ends-file", str(ends)], capture_output=True, text=True)
    assert r.returncode != 0 and "GFA 2 record type 'E'" in r.stderr


def test_gfa_crlf_and_unterminated_last_line_host_replay(cli, tmp_path):
    """CR/LF line ends are copied as read; a last line without a line feed gets one before the telomere records"""
    seq = "CCCTAA" * 20 + "ACGT" * 10
    g = tmp_path / "crlf.gfa"
    g.write_bytes(("H\tVN:Z:1.0\r\nS\tx\t%s\r\nP\tp\tx+\t*" % seq).encode())
    ends = tmp_path / "ends.tsv"
    ends.write_text("x\t120\t0\n")
    r = subprocess.run([cli, "-f", str(g), "-o", str(tmp_path), "--ends-file", str(ends)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = (tmp_path / "crlf.gfa.telo.annotated.gfa").read_bytes().decode()
    assert out == ("H\tVN:Z:1.0\r\nS\tx\t%s\r\nP\tp\tx+\t*\n"
                   "S\ttelomere_x+_start\t*\tLN:i:6\tRC:i:6000\tTL:i:120\nL\ttelomere_x+_start\t+\tx\t+\t0M\tRC:i:0\n" % seq)
