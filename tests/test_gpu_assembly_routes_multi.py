"""scanFastaToFilesDevice and annotateGfaDevice on a Teloscope of several contexts (the input's chunks dealt to all of them:
include/teloscope_mi355x_ring.hpp with detail::FastaChunkSteps and detail::GfaChunkSteps) through
tests/cpp/assembly_routes_multi_cli.cpp: 2 and 3 contexts on this one GPU against 1 context and against the host route of the
same binary — byte-equal stdout and output files, equal summary and stats structs, equal log text, equal messages — and the
per-context figures, which say that every context worked.  One set of steps serves every count (one context fills each chunk in
place, on the caller's thread and with no staging region; on several the ring deals the chunks), so 1 against N contexts compares
two ways in of one code: the independent side is the host route.  The runs go through the CLI's list mode: one process and one
Teloscope per configuration for all files and all chunk sizes of a test.  Every process is one bounded step.

The chunk count of one context is not held against the parent commit's: its loop printed no such figure (its TS_TIMING line has
stage times only), so the one-context test asserts the in-place facts — no staging, no commit, no wait, one fill per chunkBytes of
input."""
import glob
import gzip
import json
import os
import random
import shlex
import subprocess

import pytest

from tests import fastachunk as F
from tests import gfachunk as G
from tests import harness as H
from tests.test_assembly_routes_multi_cpu import build_cli
from tests.test_bam_subset import bgzf
from tests.test_fasta_chunk_reference_cpu import INPUTS
from tests.test_gfa_chunk_reference_cpu import INPUTS as GFA_INPUTS
from tests.test_gfa_mode import GFA_MANIFESTS, check_manifest, manifest_args
from tests.test_gpu_fasta_device import FLAG_SETS, HEADLINE, encodings
from tests.test_gpu_filter_device import GFA_FLAGS, PATH_GFA, PATHLESS_GFA, SHARED_GFA, gfa_filters
from tests.test_gpu_gfa_device import encodings as gfa_encodings

pytestmark = pytest.mark.gpu
MULTI = ["0,0", "0,0,0"]
TIMEOUT = 300


@pytest.fixture(scope="module")
def mcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "assembly_routes_multi_cli")


def files_of(d):
    return {os.path.relpath(p, str(d)): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(str(d), "**", "*"), recursive=True))
            if os.path.isfile(p)}


class Run:
    """One process: its exit status, stdout, the JSON lines of stderr (one per file and chunk size), the other stderr lines and
    the files it wrote, by their path under the output directory."""

    def __init__(self, mcli, out, fmt, route, devices, flags, inputs, chunks=None):
        os.makedirs(str(out), exist_ok=True)
        cmd = [mcli, fmt, route, "-o", os.path.join(str(out), "files")] + [str(f) for f in flags]
        cmd += (["--devices", devices] if devices else []) + (["--chunk-bytes", ",".join(str(c) for c in chunks)] if chunks else [])
        if isinstance(inputs, (list, tuple)):
            with open(os.path.join(str(out), "list.txt"), "w") as fh:
                fh.write("".join(str(p) + "\n" for p in inputs))
            cmd += ["--each", os.path.join(str(out), "list.txt")]
        else:
            cmd.append(str(inputs))
        r = subprocess.run(cmd, stdin=subprocess.DEVNULL, capture_output=True, timeout=TIMEOUT)
        self.returncode, self.stdout, self.stderr = r.returncode, r.stdout, r.stderr
        lines = r.stderr.decode(errors="replace").splitlines()
        self.records = [json.loads(l) for l in lines if l.startswith("{")]
        self.other = [l for l in lines if not l.startswith("{")]
        self.files = files_of(os.path.join(str(out), "files"))
        assert r.returncode in (0, 1), (cmd, r.returncode, r.stderr[-500:])

    def by_chunk(self, chunk, many):
        """The files of one chunk size, by their path under that size's directory."""
        if not many:
            return self.files
        prefix = "c%d/" % chunk
        return {f[len(prefix):]: v for f, v in self.files.items() if f.startswith(prefix)}


def comparable(record):
    """A file's JSON record without what may differ between configurations: the per-context figures."""
    return {k: v for k, v in record.items() if k not in ("contexts", "route")}


def assert_same_files(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want))[:6])
    for name in want:
        assert got[name] == want[name], (what, name)


# ------------------------------------------------------------------------------------------------------------ FASTA
FASTA_CHUNKS = [64, 257, 4096]
# the committed files of 2 to 8 KB go through chunks of 64, 257 and 4 096 bytes; the two gzipped assemblies, one record of 4 MB
# each, through chunks of 4 096 bytes only, where each of them spans a thousand chunks already (at 64 bytes it would be 65 000
# chunks per run: minutes, not seconds)
SMALL = [p for p in INPUTS if not p.endswith(".gz")]
LARGE = [p for p in INPUTS if p.endswith(".gz")]
_host_runs = {}


def fasta_host(mcli, root, name, which, inputs):
    """The host route's run over committed FASTA files under a flag set: computed once, left unchanged."""
    if (name, which) not in _host_runs:
        r = Run(mcli, root / ("host_%s_%s" % (which, name.replace(" ", "_"))), "--fasta", "--host", None, shlex.split(FLAG_SETS[name]), inputs)
        assert r.returncode == 0, r.stderr[-500:]
        _host_runs[(name, which)] = r
    return _host_runs[(name, which)]


@pytest.fixture(scope="module")
def fasta_root(tmp_path_factory):
    return tmp_path_factory.mktemp("fasta")


@pytest.mark.parametrize("tracks", [False, True], ids=["records", "device-tracks"])
@pytest.mark.parametrize("name", sorted(FLAG_SETS))
def test_fasta_byte_for_byte(mcli, fasta_root, name, tracks):
    """Every committed FASTA under the six flag sets of tests/test_gpu_fasta_device.py, each also with --device-tracks: 1, 2 and 3
    contexts give the host route's stdout and files, and 2 and 3 give one context's summary and the deterministic fields of
    ScanFastaTimes.  At 64 and 257 bytes every record of the small files spans many chunks and contexts; at 4 096 multi.fa puts
    several records in one chunk, and the records of the two gzipped assemblies span a thousand chunks.  Under every flag set,
    the list and the wide form among them, context 1 scanned bases."""
    assert len(SMALL) >= 30 and len(LARGE) == 2
    flags = shlex.split(FLAG_SETS[name]) + (["--device-tracks"] if tracks else [])
    for which, inputs, chunks in (("small", SMALL, FASTA_CHUNKS), ("large", LARGE, [4096])):
        host = fasta_host(mcli, fasta_root, name, which, inputs)
        many = len(chunks) > 1
        tag = "%s_%s_%d" % (which, name.replace(" ", "_"), tracks)
        runs = {d: Run(mcli, fasta_root / (tag + "_" + d.replace(",", "")), "--fasta", "--device", d, flags, inputs, chunks) for d in ["0"] + MULTI}
        one = runs["0"]
        for devices, r in runs.items():
            assert r.returncode == 0 and not r.other, (devices, r.other[-3:])
            assert r.stdout == host.stdout * len(chunks), (which, devices)
            for chunk in chunks:
                assert_same_files(r.by_chunk(chunk, many), host.files, (which, devices, chunk))
            assert len(r.records) == len(chunks) * len(inputs)
            assert [comparable(x) for x in r.records] == [comparable(x) for x in one.records], (which, devices)
            for x in r.records:
                assert len(x["contexts"]) == len(devices.split(","))
                assert sum(c["basesScanned"] for c in x["contexts"]) == x["times"]["library_bases"]
        assert {x["times"]["bases"] for x in one.records} != {0}
        if "-m" in FLAG_SETS[name]:
            assert any(x["times"]["bases_read_back"] for x in one.records) != tracks       # (with device tracks no base is read back)
        for devices in MULTI:
            assert sum(x["contexts"][1]["basesScanned"] for x in runs[devices].records) > 0, (name, devices)


def test_fasta_encodings(mcli, tmp_path):
    """A dozen files as plain, bgzip with small members (several per chunk), bgzip then gzip, gzip, CRLF and lower case at chunks
    of 4096 bytes: 2 and 3 contexts give the host route's and one context's bytes."""
    plain = [p for p in INPUTS if not p.endswith(".gz")]
    picked = [p for p in plain if os.path.basename(p).startswith(("gapped_", "multi"))][:8] + plain[:4]
    assert len(set(picked)) == 12
    inputs = []
    for k, p in enumerate(sorted(set(picked))):
        inputs += encodings(tmp_path, "f%02d" % k, open(p, "rb").read())
    flags = shlex.split(HEADLINE)
    host = Run(mcli, tmp_path / "host", "--fasta", "--host", None, flags, inputs)
    one = Run(mcli, tmp_path / "one", "--fasta", "--device", "0", flags, inputs, [4096])
    assert host.returncode == one.returncode == 0, (host.stderr[-300:], one.stderr[-300:])
    for devices in MULTI:
        r = Run(mcli, tmp_path / devices.replace(",", ""), "--fasta", "--device", devices, flags, inputs, [4096])
        assert r.returncode == 0 and not r.other, r.other[-3:]
        assert r.stdout == host.stdout == one.stdout
        assert_same_files(r.files, host.files, devices)
        assert_same_files(r.files, one.files, devices)
        assert [comparable(x) for x in r.records] == [comparable(x) for x in one.records]


def spanning_assembly():
    """Four records of about 50 KB: N-runs of 1 500 bases and telomeres of 1 800, each longer than a chunk of 1 024 bytes, so that
    every one of them straddles at least one chunk cut; lines of 60."""
    gen = random.Random(41)
    out = []
    for i in range(4):
        body = b"CCCTAA" * 300
        for _ in range(6):
            body += F.random_bases(gen, 6000, gaps=False) + b"N" * 1500
        body += F.random_bases(gen, 3000, gaps=False) + b"TTAGGG" * 300
        out.append(F.record_text(b"spanning_%d some words" % i, body, 60))
    return b"".join(out)


@pytest.mark.parametrize("tracks", [False, True], ids=["records", "device-tracks"])
def test_fasta_record_across_many_chunks_with_gaps(mcli, tmp_path, tracks):
    """About 200 KB at chunks of 1 024 bytes under the headline flags with -m: every record spans about 50 chunks and every
    context, with N-runs and telomeres across the cuts."""
    text = spanning_assembly()
    assert 190_000 < len(text) < 230_000
    p = tmp_path / "spanning.fa"
    p.write_bytes(text)
    flags = shlex.split(HEADLINE) + (["--device-tracks"] if tracks else [])
    host = Run(mcli, tmp_path / "host", "--fasta", "--host", None, shlex.split(HEADLINE), [p])
    one = Run(mcli, tmp_path / "one", "--fasta", "--device", "0", flags, [p], [1024])
    assert host.returncode == one.returncode == 0, (host.stderr[-300:], one.stderr[-300:])
    assert host.files["0.spanning.fa_gaps.bed"].count(b"\n") == 24
    assert host.files["0.spanning.fa_terminal_telomeres.bed"].count(b"\n") >= 8 and host.files["0.spanning.fa_canonical_matches.bed"]
    for devices in MULTI:
        r = Run(mcli, tmp_path / devices.replace(",", ""), "--fasta", "--device", devices, flags, [p], [1024])
        assert r.returncode == 0 and not r.other, r.other[-3:]
        assert r.stdout == host.stdout == one.stdout
        assert_same_files(r.files, host.files, devices)
        assert comparable(r.records[0]) == comparable(one.records[0])
        assert all(c["chunks"] > 50 for c in r.records[0]["contexts"])


@pytest.fixture(scope="module")
def many_records(tmp_path_factory):
    p = tmp_path_factory.mktemp("many") / "many.fa"
    p.write_bytes(F.assembly_text(43, 60, lo=200, hi=3000))
    return p


@pytest.mark.parametrize("devices", MULTI)
def test_fasta_every_context_works(mcli, tmp_path, many_records, devices):
    """Fails without the feature (the call threw).  60 records in about 90 chunks of 1 024 bytes: every context took chunks, framed
    records and scanned, the chunk counts differ by one at the most, and the sums are the input's."""
    n = len(devices.split(","))
    size = os.path.getsize(str(many_records))
    n_chunks = -(-size // 1024)
    assert n_chunks >= 3 * n
    one = Run(mcli, tmp_path / "one", "--fasta", "--device", "0", shlex.split(HEADLINE), [many_records], [1024])
    r = Run(mcli, tmp_path / "multi", "--fasta", "--device", devices, shlex.split(HEADLINE), [many_records], [1024])
    assert r.returncode == one.returncode == 0, (r.stderr[-300:], one.stderr[-300:])
    ctx = r.records[0]["contexts"]
    print(json.dumps(ctx))
    assert len(ctx) == n and [c["device"] for c in ctx] == [0] * n
    assert all(c["chunks"] > 0 and c["records"] > 0 and c["basesScanned"] > 0 for c in ctx)
    assert max(c["chunks"] for c in ctx) - min(c["chunks"] for c in ctx) <= 1
    assert sum(c["chunks"] for c in ctx) == n_chunks
    assert sum(c["records"] for c in ctx) == 60 == r.records[0]["summary"]["totalPaths"]
    assert sum(c["basesScanned"] for c in ctx) == one.records[0]["times"]["library_bases"] > 0
    assert sum(c["bytesReceived"] for c in ctx) == size
    assert all(c["msFill"] == 0 and c["msStage"] > 0 and c["msCommit"] > 0 for c in ctx)


def test_fasta_one_context_fills_in_place(mcli, tmp_path, many_records):
    """One context: no staging, no commit and no wait for a serial section; one fill per chunkBytes of input."""
    size = os.path.getsize(str(many_records))
    one = Run(mcli, tmp_path / "one", "--fasta", "--device", "0", shlex.split(HEADLINE), [many_records], [1024])
    assert one.returncode == 0, one.stderr[-300:]
    (c,) = one.records[0]["contexts"]
    print(json.dumps(c))
    assert c["msStage"] == 0 and c["msCommit"] == 0 and c["msFrameWait"] == 0 and c["msFill"] > 0
    assert c["chunks"] == -(-size // 1024) and c["records"] == 60 and c["bytesReceived"] == size
    # no --devices at all is the same route
    bare = Run(mcli, tmp_path / "bare", "--fasta", "--device", None, shlex.split(HEADLINE), [many_records], [1024])
    assert bare.stdout == one.stdout and bare.files == one.files and len(bare.records[0]["contexts"]) == 1


def test_fasta_failures_alike(mcli, tmp_path):
    """A BGZF member with a wrong CRC in a middle chunk, a truncated BGZF file, a truncated gzip and a record in a later chunk
    that does not fit --chunk-limit: the same exit status, the same message and, where the file is read, the same bytes on 1, 2
    and 3 contexts, every run within its timeout."""
    text = F.assembly_text(44, 30, lo=500, hi=3000)
    good = bytearray(bgzf(text, 3000))
    at, members = 0, []
    while at < len(good):
        members.append(at)
        at += int.from_bytes(good[at + 16:at + 18], "little") + 1
    assert len(members) > 12
    crc = bytearray(good)
    crc[members[7] - 8] ^= 0xff                                     # the CRC32 of member 6, in the middle of the input
    big = b"".join(F.record_text(b"small_%d" % i, b"ACGT" * 100) for i in range(12)) + F.record_text(b"too_big some words", b"ACGT" * 2500) + \
        F.record_text(b"after", b"ACGT" * 10)
    cases = {"crc.fa.gz": bytes(crc), "cut_bgzf.fa.gz": bytes(good[:members[6] + 40]), "cut_gzip.fa.gz": gzip.compress(text, 6)[:-3000], "big_record.fa": big}
    paths = []
    for name, data in cases.items():
        (tmp_path / name).write_bytes(data)
        paths.append(tmp_path / name)
    flags = ["--chunk-limit", "5000"]
    runs = {d: Run(mcli, tmp_path / d.replace(",", ""), "--fasta", "--device", d, flags, paths, [700]) for d in ["0"] + MULTI}
    one = runs["0"]
    assert one.returncode == 1 and len(one.records) == 4, one.stderr[-600:]
    errors = {x["file"]: x.get("error") for x in one.records}
    print(json.dumps(errors))
    assert errors["crc.fa.gz"] == "BGZF checksum mismatch"
    assert errors["big_record.fa"] == "FASTA record 'too_big' does not fit a device chunk (5000 bytes of text); use the host route"
    # (zlib's streaming reader takes what a truncated stream still gives and ends there, as tests/test_gpu_gzip_feed.py and
    # tests/test_gpu_fastq_device.py hold for every route that reads through it: these two end alike, without a message)
    assert errors["cut_gzip.fa.gz"] is None and errors["cut_bgzf.fa.gz"] is None
    for devices in MULTI:
        r = runs[devices]
        assert r.returncode == 1
        assert {x["file"]: x.get("error") for x in r.records} == errors, devices
        assert r.other == one.other and r.stdout == one.stdout
        assert [comparable(x) for x in r.records] == [comparable(x) for x in one.records]
        for f in one.files:                                         # (what a failed file left behind is not compared)
            if f.startswith(("1.", "2.")):
                assert r.files[f] == one.files[f], (devices, f)
    assert any(f.startswith("1.") for f in one.files) and one.records[1]["summary"]["totalPaths"] > 3
    # ... and with room for the record every configuration reads the file
    fits = [Run(mcli, tmp_path / ("fits" + d.replace(",", "")), "--fasta", "--device", d, ["--chunk-limit", "20000"], [paths[3]], [700]) for d in ["0"] + MULTI]
    assert all(r.returncode == 0 and r.stdout == fits[0].stdout and r.files == fits[0].files for r in fits)
    assert fits[0].records[0]["summary"]["totalPaths"] == 14


def test_filtered_fasta_on_several_contexts_is_refused(mcli, tmp_path):
    """The filtered device route runs on one device: with a selector and two contexts the call says so before any output file
    exists; on one context it selects."""
    multi = H.golden_path("testFiles/multi.fa")
    r = Run(mcli, tmp_path / "two", "--fasta", "--device", "0,0", ["--include-prefix", "contig_t2t"], multi)
    assert r.returncode == 1 and not r.files and r.stdout == b""
    assert len(r.other) == 1 and r.other[0].startswith("Error: scanFastaToFilesDevice with assembly record filters runs on one device: "
                                                       "this Teloscope was made over 2"), r.other
    assert "the filtered device route" in r.other[0]
    r = Run(mcli, tmp_path / "one", "--fasta", "--device", "0", ["--include-prefix", "contig_t2t"], multi)
    assert r.returncode == 0 and r.records[0]["log"] == "Sequence filter: selected 1 of 3 paths.\n" and r.files


# ------------------------------------------------------------------------------------------------------------ GFA
GFA_CHUNKS = [64, 4096]


def spread_graph():
    """A graph whose P lines come first, with an S line longer than several chunks of 4 096 bytes, and whose paths end in segments
    that lie far apart in the text: 40 segments of 1 to 3 KB, one of 20 KB, 6 paths."""
    gen = random.Random(45)
    names = [b"s%d" % i for i in range(40)]
    lines = [b"H\tVN:Z:1.0\n"]
    for k in range(6):
        comps = [names[k], names[20 + k], names[39 - k]]
        lines.append(b"P\tpath%d\t%s\t*\n" % (k, b",".join(c + b"+" for c in comps)))
    for i, nm in enumerate(names):
        n = 20_000 if i == 17 else gen.randrange(1000, 3000)
        lines.append(b"S\t%s\t%s\n" % (nm, G.bases(gen, n, ("start", "end", "both", None)[i % 4])))
    return b"".join(lines)


def gfa_inputs(tmp_path):
    """The 16 committed graphs as plain, bgzip, bgzip then gzip, gzip and CRLF, the generators of tests/test_gpu_gfa_device.py
    (at a size that chunks of 64 bytes go through in seconds) and the spread graph."""
    inputs = []
    for k, p in enumerate(GFA_INPUTS):
        inputs += gfa_encodings(tmp_path, "g%02d" % k, open(p, "rb").read())
    for name, text in (("pathless.gfa", G.pathless_graph(11, 60, 50, 600)), ("paths.gfa", G.path_graph(12, 80, 8, 100, 500)), ("spread.gfa", spread_graph())):
        (tmp_path / name).write_bytes(text)
        inputs.append(tmp_path / name)
    inputs += gfa_encodings(tmp_path, "spread", spread_graph())[1:4]
    return inputs


def gfa_comparable(run):
    return [comparable(x) for x in run.records]


def test_gfa_byte_for_byte(mcli, tmp_path):
    """Both output files, the log text and GfaAnnotateStats on 2 and 3 contexts at chunks of 64 and 4 096 bytes: the host route's
    and one context's.  In the spread graph the wanted segments lie on at least two contexts, which the per-context figures and
    terminalEndsStats of every context say."""
    assert len(GFA_INPUTS) == 16
    inputs = gfa_inputs(tmp_path)
    host = Run(mcli, tmp_path / "host", "--gfa", "--host", None, GFA_FLAGS, inputs)
    one = Run(mcli, tmp_path / "one", "--gfa", "--device", "0", GFA_FLAGS, inputs, GFA_CHUNKS)
    assert host.returncode == one.returncode == 0, (host.stderr[-300:], one.stderr[-300:])
    assert any(x["log"] for x in host.records) and any(b"telomere_" in v for v in host.files.values())
    host_view = [{k: v for k, v in comparable(x).items() if k != "chunkBytes"} for x in host.records]
    for devices in ["0"] + MULTI:
        r = one if devices == "0" else Run(mcli, tmp_path / devices.replace(",", ""), "--gfa", "--device", devices, GFA_FLAGS, inputs, GFA_CHUNKS)
        n = len(devices.split(","))
        assert r.returncode == 0 and r.other == host.other * len(GFA_CHUNKS), (devices, r.other[-3:])
        assert r.stdout == host.stdout * len(GFA_CHUNKS)
        assert gfa_comparable(r) == gfa_comparable(one)
        for k, chunk in enumerate(GFA_CHUNKS):
            assert_same_files(r.by_chunk(chunk, True), host.files, (devices, chunk))
            got = [{a: b for a, b in comparable(x).items() if a != "chunkBytes"} for x in r.records[k * len(inputs):(k + 1) * len(inputs)]]
            assert got == host_view, (devices, chunk)
        for x in r.records:
            ctx = x["contexts"]
            assert len(ctx) == n
            assert sum(c["records"] for c in ctx) == x["stats"]["segments"]
            # one terminalEnds call per context that owns a wanted segment: its segments went one of the three ways
            assert sum(sum(c["terminalEnds"][:3]) for c in ctx) == x["stats"]["scanned"]
            assert all(sum(c["terminalEnds"][:3]) > 0 for c in ctx if c["basesScanned"] > 0)
        if n > 1:
            for chunk in GFA_CHUNKS:
                (x,) = [x for x in r.records if x["file"] == "spread.gfa" and x["chunkBytes"] == chunk]
                print(devices, chunk, json.dumps(x["contexts"]))
                assert x["stats"]["scanned"] >= 12 and sum(1 for c in x["contexts"] if c["basesScanned"] > 0) >= 2
                assert all(c["chunks"] > 0 for c in x["contexts"])


def manifest_groups():
    """The GFA manifests by their flags (everything but the input and the output directory), so that one process serves a group."""
    groups = {}
    for path in GFA_MANIFESTS:
        m = H.load_manifest(path)
        args = manifest_args(m, "%OUT%")
        src = args[args.index("-f") + 1]
        flags, skip = [], False
        for a in args:
            if skip:
                skip = False
            elif a in ("-f", "-o", "-j"):
                skip = True
            else:
                flags.append(a)
        groups.setdefault(tuple(flags), []).append((path, m, src))
    return groups


def test_gfa_manifests(mcli, tmp_path):
    """Every GFA manifest on 2 and 3 contexts at chunks of 64 and 4 096 bytes: the host route's and one context's files, and the
    manifest's own expectations."""
    assert len(GFA_MANIFESTS) == 15
    for g, (flags, members) in enumerate(sorted(manifest_groups().items())):
        inputs = [src for _, _, src in members]
        host = Run(mcli, tmp_path / ("host%d" % g), "--gfa", "--host", None, flags, inputs)
        assert host.returncode == 0, host.stderr[-300:]
        one = None
        for devices in ["0"] + MULTI:
            out = tmp_path / ("g%d_%s" % (g, devices.replace(",", "")))
            r = Run(mcli, out, "--gfa", "--device", devices, flags, inputs, GFA_CHUNKS)
            one = one or r
            assert r.returncode == 0 and r.other == host.other * len(GFA_CHUNKS), (devices, r.other[-3:])
            assert r.stdout == host.stdout * len(GFA_CHUNKS) and gfa_comparable(r) == gfa_comparable(one)
            for chunk in GFA_CHUNKS:
                assert_same_files(r.by_chunk(chunk, True), host.files, (flags, devices, chunk))
                for k, (path, m, src) in enumerate(members):
                    check_manifest(m, src, os.path.join(str(out), "files", "c%d" % chunk, str(k)), 0, r.stderr.decode())
                    if os.path.basename(path) == "gfa_noseq_small.tst":
                        assert "2 of 2 GFA segment(s) had no sequence" in r.records[(0 if chunk == 64 else len(inputs)) + k]["log"]


def offence_graphs():
    """Two offences in different chunks (of 64 and of 4 096 bytes alike: 5 KB of sequence lie between them): the first by line
    number is the one reported, whichever context framed it.  -> name -> (text, message)"""
    gen = random.Random(46)
    seq = G.bases(gen, 5000, "start")
    gfa2 = "; use GFA1 P paths or a pathless GFA1 graph."
    return {
        "w_then_c.gfa": (b"S\ta\t" + seq + b"\nW\tw\t0\tc\t0\t4\t>a\nS\tb\t" + seq + b"\nC\ta\t+\tb\t+\t0\t2M\nS\tc\tACGT\n",
                         "Assembly record filters do not support GFA1 W walks at line 2" + gfa2),
        "c_then_w.gfa": (b"S\ta\tACGT\nS\tb\t" + seq + b"\nC\ta\t+\tb\t+\t0\t2M\nS\tc\t" + seq + b"\nW\tw\t0\tc\t0\t4\t>a\n",
                         "Assembly record filters do not support GFA1 C containment records at line 3."),
        "offence_and_twice.gfa": (b"S\ta\t" + seq + b"\nS\ta\t" + seq + b"\nX\tfoo\n", "Assembly record filters do not support GFA record type 'X' at line 3."),
    }


@pytest.mark.parametrize("gfa", [PATH_GFA, PATHLESS_GFA, SHARED_GFA], ids=["paths", "pathless", "shared"])
def test_gfa_with_selectors(mcli, tmp_path, gfa):
    """The three filter graphs of tests/test_gpu_filter_device.py with their selector options on 2 contexts at chunks of 64 and
    4 096 bytes: one context's files, stats and `Sequence filter:` line, which are the host route's."""
    for k, filters in enumerate(gfa_filters(tmp_path, gfa)):
        tag = "s%d" % k
        host = Run(mcli, tmp_path / (tag + "host"), "--gfa", "--host", None, GFA_FLAGS + filters, [gfa])
        one = Run(mcli, tmp_path / (tag + "one"), "--gfa", "--device", "0", GFA_FLAGS + filters, [gfa], GFA_CHUNKS)
        two = Run(mcli, tmp_path / (tag + "two"), "--gfa", "--device", "0,0", GFA_FLAGS + filters, [gfa], GFA_CHUNKS)
        assert host.returncode == one.returncode == two.returncode == 0, (host.stderr[-300:], one.stderr[-300:], two.stderr[-300:])
        assert host.records[0]["log"].startswith("Sequence filter: selected ")
        assert gfa_comparable(two) == gfa_comparable(one) and two.stdout == one.stdout == host.stdout * 2
        for x in two.records:
            assert x["log"] == host.records[0]["log"] and x["stats"] == host.records[0]["stats"]
        for chunk in GFA_CHUNKS:
            assert_same_files(two.by_chunk(chunk, True), host.files, (tag, chunk))
            assert_same_files(one.by_chunk(chunk, True), host.files, (tag, chunk))


def test_gfa_refusals_with_selectors(mcli, tmp_path):
    """Offences in different chunks, so on different contexts: the first by line number wins over a later one, whichever was
    framed where, and over the graph build's errors — the host route's and one context's message."""
    cases = offence_graphs()
    paths = []
    for name, (text, _) in cases.items():
        (tmp_path / name).write_bytes(text)
        paths.append(tmp_path / name)
    flags = GFA_FLAGS + ["--include-prefix", "a"]
    host = Run(mcli, tmp_path / "refused_host", "--gfa", "--host", None, flags, paths)
    for devices in ("0", "0,0", "0,0,0"):
        r = Run(mcli, tmp_path / ("refused" + devices.replace(",", "")), "--gfa", "--device", devices, flags, paths, GFA_CHUNKS)
        assert r.returncode == host.returncode == 1 and not r.files and r.stdout == b""
        assert [x["error"] for x in r.records] == [m for _, m in cases.values()] * 2, devices
        assert [x["error"] for x in host.records] == [m for _, m in cases.values()]
        assert r.other == host.other * 2


def test_gfa_error_cases(mcli, tmp_path):
    """The error cases of tests/test_gpu_gfa_device.py on 2 contexts: the host route's and one context's message and exit status,
    and no output file."""
    e = G.edge_cases()
    wanted = (("duplicate segment name", "segment 'b' is defined twice"), ("gfa2 with an E record", "GFA 2 record type 'E'"),
              ("gfa2 whose first foreign line is not its first", "GFA 2 record type 'GG'"))
    paths = []
    for name, _ in wanted:
        p = tmp_path / (name.replace(" ", "_") + ".gfa")
        p.write_bytes(e[name])
        paths.append(p)
    paths.append(tmp_path / "is_not_there.gfa")
    flipped = bytearray(bgzf(G.path_graph(14, 60, 6), 3000))
    flipped[18 + 40] ^= 0x10                                        # inside the first member's deflate payload
    host = Run(mcli, tmp_path / "host", "--gfa", "--host", None, [], paths)
    one = Run(mcli, tmp_path / "one", "--gfa", "--device", "0", [], paths, GFA_CHUNKS)
    two = Run(mcli, tmp_path / "two", "--gfa", "--device", "0,0", [], paths, GFA_CHUNKS)
    assert host.returncode == one.returncode == two.returncode == 1
    assert not two.files and two.stdout == b""
    errors = [x["error"] for x in host.records]
    for (name, msg), got in zip(wanted, errors):
        assert msg in got, name
    assert "Could not open assembly input" in errors[3]
    assert [x["error"] for x in two.records] == [x["error"] for x in one.records] == errors * 2
    assert two.other == one.other == host.other * 2
    (tmp_path / "flipped.gfa.gz").write_bytes(bytes(flipped))
    runs = [Run(mcli, tmp_path / ("flipped" + d.replace(",", "")), "--gfa", "--device", d, [], tmp_path / "flipped.gfa.gz", [4096]) for d in ("0", "0,0")]
    assert runs[0].returncode == runs[1].returncode == 1 and runs[0].other == runs[1].other
    assert runs[1].other[0][7:] in ("invalid BGZF deflate payload", "BGZF checksum mismatch")
