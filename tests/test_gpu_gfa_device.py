"""The device route of the GFA annotation (annotateGfaDevice: the graph's text inflated, indexed and framed on the GPU, every
wanted segment scanned where it lies in device memory) through tests/cpp/gfa_device_cli.cpp: --device against --host of the same
binary on the same inputs — the same exit status, the same stdout apart from the three time fields, byte-equal stderr and
byte-equal output files.  The stage is compared with a plain reference in tests/test_gpu_gfa_chunk.py.  Every process is one
bounded step."""
import glob
import gzip
import os
import random
import subprocess

import pytest

from tests import gfachunk as G
from tests import harness as H
from tests.test_bam_subset import EOF_BLOCK, bgzf, bgzf_fancy
from tests.test_gfa_chunk_reference_cpu import INPUTS, build_cli
from tests.test_gfa_mode import GFA_MANIFESTS, IDS, check_manifest, manifest_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "gfa_device_cli")


def files_of(d):
    return {os.path.relpath(p, str(d)): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(str(d), "**", "*"), recursive=True))
            if os.path.isfile(p)}


def without_times(stdout):
    """The stats lines without their last three fields (parse, scan and write milliseconds)."""
    return [line.split()[:-3] for line in stdout.split(b"\n") if line]


def both(dcli, tmp_path, flags, inputs, tag="run", timeout=300, extra_device=()):
    """The device run and the host run of the same command over `inputs` (one path through -f, or a list through --each): equal
    exit status, stdout equal apart from the times, byte-equal stderr and output files; -> (device result, the device run's files)."""
    res, outs = [], []
    for route in ("--device", "--host"):
        out = tmp_path / ("%s%s" % (tag, route))
        cmd = [dcli, route] + list(flags) + (list(extra_device) if route == "--device" else [])
        if "-o" not in cmd:
            cmd += ["-o", str(out)]
        if isinstance(inputs, (list, tuple)):
            lst = tmp_path / (tag + ".list")
            lst.write_text("".join(str(p) + "\n" for p in inputs))
            cmd += ["--each", str(lst)]
        elif inputs is not None:
            cmd += ["-f", str(inputs)]
        os.makedirs(str(out), exist_ok=True)
        res.append(subprocess.run([c.replace("%ROUTE%", str(out)) for c in cmd], stdin=subprocess.DEVNULL, capture_output=True, timeout=timeout))
        outs.append(files_of(out))
    d, h = res
    assert d.returncode in (0, 1) and h.returncode in (0, 1), (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert d.returncode == h.returncode, (d.returncode, h.returncode, d.stderr[-300:], h.stderr[-300:])
    assert without_times(d.stdout) == without_times(h.stdout)
    assert d.stderr == h.stderr, (d.stderr[-300:], h.stderr[-300:])
    assert sorted(outs[0]) == sorted(outs[1])
    for name in outs[1]:
        assert outs[0][name] == outs[1][name], name
    return d, outs[0]


@pytest.mark.parametrize("path", GFA_MANIFESTS, ids=IDS)
def test_gfa_manifest_through_the_device_route(dcli, tmp_path, path):
    m = H.load_manifest(path)
    args = [("%ROUTE%" if a == "%OUT%" else a) for a in manifest_args(m, "%OUT%")]
    d, _ = both(dcli, tmp_path, args, None)
    check_manifest(m, args[args.index("-f") + 1], str(tmp_path / "run--device"), d.returncode, d.stderr.decode())
    if os.path.basename(path) == "gfa_noseq_small.tst":
        assert b"2 of 2 GFA segment(s) had no sequence" in d.stderr


def encodings(tmp_path, tag, text):
    """The text as a plain file, bgzipped, bgzipped and then plain-gzipped, plain-gzipped and with CRLF line ends."""
    half = len(text) // 2
    half = text.index(b"\n", half) + 1 if b"\n" in text[half:] else half
    out = []
    for name, data in (("plain", text), ("bgzf", bgzf_fancy(text, 1777, random.Random(5))),
                       ("bgzf_then_gzip", bgzf(text[:half], 3000)[:-len(EOF_BLOCK)] + gzip.compress(text[half:], 1)),
                       ("gzip", gzip.compress(text, 6)), ("crlf", G.crlf(text))):
        p = tmp_path / ("%s.%s.gfa" % (tag, name))
        p.write_bytes(data)
        out.append(p)
    return out


@pytest.mark.parametrize("chunk", [None, 4096])
def test_every_committed_graph_in_every_encoding(dcli, tmp_path, chunk):
    """All 16 committed graphs, each plain, bgzipped, bgzipped then gzipped, gzipped and with CRLF, through one Teloscope per
    route; every compressed encoding of a graph gives the plain file's outputs."""
    assert len(INPUTS) == 16
    inputs = []
    for k, p in enumerate(INPUTS):
        inputs += encodings(tmp_path, "g%02d" % k, open(p, "rb").read())
    d, files = both(dcli, tmp_path, ["--chunk-bytes", str(chunk)] if chunk else [], inputs)
    assert d.returncode == 0, d.stderr[-300:]
    assert len(files) == 2 * len(inputs)
    for k in range(16):
        want = None
        for i in range(5 * k, 5 * k + 4):                          # (CRLF keeps its line ends: its bytes differ)
            got = sorted(v for f, v in files.items() if f.startswith("%d/" % i))
            assert len(got) == 2
            want = got if want is None else want
            assert got == want, inputs[i]
    assert any(b"telomere_" in v for v in files.values())


def test_generated_graphs(dcli, tmp_path):
    """Two graphs of about 2 MB at 64 KB chunks: 3 000 pathless segments, a tenth of them telomere-capped; and one with paths whose
    P lines stand first and whose H line stands last."""
    a, b = tmp_path / "pathless.gfa", tmp_path / "paths.gfa"
    a.write_bytes(G.pathless_graph(11, 3000, 50, 2000))
    b.write_bytes(G.path_graph(12, 1200, 40, 200, 3000))
    assert a.stat().st_size > 2_000_000 and b.stat().st_size > 1_500_000
    d, files = both(dcli, tmp_path, ["--chunk-bytes", "65536"], [a, b, *encodings(tmp_path, "p", b.read_bytes())[1:3]])
    assert d.returncode == 0, d.stderr[-300:]
    rows = without_times(d.stdout)
    assert rows[0][:3] == [b"3000", b"3000", b"3000"] and int(rows[0][4]) >= 100
    assert rows[1][0] == b"1200" and rows[1][1] == rows[1][2] == b"80" and int(rows[1][4]) >= 40
    assert rows[2] == rows[1] == rows[3]


def test_one_long_line_grows_the_chunk(dcli, tmp_path):
    gen = random.Random(13)
    p = tmp_path / "long.gfa"
    p.write_bytes(b"H\tVN:Z:1.0\nS\tshort\t%s\nS\tlong\t%s\tLN:i:300000\nS\tafter\t%s\n" % (
        G.bases(gen, 500, "end"), G.bases(gen, 300_000, "both"), G.bases(gen, 700, "start")))
    d, files = both(dcli, tmp_path, ["--chunk-bytes", "4096"], p)
    assert d.returncode == 0, d.stderr[-300:]
    assert without_times(d.stdout)[0][:3] == [b"3", b"3", b"3"]
    assert b"telomere_long+_start" in files["long.gfa.telo.annotated.gfa"] and b"telomere_long+_end" in files["long.gfa.telo.annotated.gfa"]


def test_errors_are_the_host_routes(dcli, tmp_path):
    e = G.edge_cases()
    for name, msg in (("duplicate segment name", b"segment 'b' is defined twice"), ("gfa2 with an E record", b"GFA 2 record type 'E'"),
                      ("gfa2 whose first foreign line is not its first", b"GFA 2 record type 'GG'")):
        p = tmp_path / (name.replace(" ", "_") + ".gfa")
        p.write_bytes(e[name])
        for flags in ([], ["--chunk-bytes", "64"]):
            d, files = both(dcli, tmp_path, flags, p, tag=p.name + str(len(flags)))
            assert d.returncode == 1 and d.stderr.startswith(b"Error: ") and msg in d.stderr and not files, (name, d.stderr[-300:])
    d, _ = both(dcli, tmp_path, [], tmp_path / "is_not_there.gfa", tag="missing")
    assert d.returncode == 1 and b"Could not open assembly input" in d.stderr


def test_two_ordinals_are_refused(dcli, tmp_path):
    """Two contexts on this one GPU are several devices, as far as the route can tell; the host route takes them."""
    g = H.golden_path("testFiles/gfa_telo.gfa")
    r = subprocess.run([dcli, "--device", "--devices", "0,0", "-o", str(tmp_path), "-f", g], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"runs on one device" in r.stderr and b"made over 2" in r.stderr, r.stderr[-300:]
    r = subprocess.run([dcli, "--host", "--devices", "0,0", "-o", str(tmp_path), "-f", g], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]


def test_damaged_bgzf_is_an_error_not_a_signal(dcli, tmp_path):
    """A flipped payload byte in a bgzipped graph: the device run exits 1 with the BAM route's message (the host route reads the
    same file through zlib, whose words differ: DESIGN, FASTQ on the device)."""
    good = bytearray(bgzf(G.path_graph(14, 60, 6), 3000))
    good[18 + 40] ^= 0x10                                           # inside the first member's deflate payload
    p = tmp_path / "flipped.gfa.gz"
    p.write_bytes(bytes(good))
    r = subprocess.run([dcli, "--device", "-o", str(tmp_path / "out"), "-f", str(p)], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and r.stderr[7:].strip() in (b"invalid BGZF deflate payload", b"BGZF checksum mismatch"), r.stderr[-200:]
