"""The parallel record index of a resident BAM chunk (ts_bam_chunk_index) on the device, stage by stage: its table, next, error
and error_off against ts_bam_chunk_walk on the same chunk, against ref_walk and against the plain-Python model of the scheme
(tests/bamindex.py, pinned without a device by tests/test_bam_index_cpu.py), and its statistics against the model's — at the
smallest shapes at which spans, candidates and the chain can go wrong (ts_bam_chunk_set_index_geometry: spans of 64 bytes and
more, 1 and 4 candidates).  Then the route: tests/cpp/bam_index_cli.cpp with --walk index writes the bytes of --walk serial and
of the host route.  Equality is exact everywhere."""
import ctypes as C
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from tests import bamchunk as B
from tests import bamindex as I
from tests import harness as H
from tests import seqgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_BYTES = 8 << 20
BIG = 1 << 20


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    rf = ta.ReadTelomereFilter(user_input(H.parse_cli("--fastq-subset -l 42"), device=0))
    chunk = B.Chunk(rf._ctx.ptr, CHUNK_BYTES, CHUNK_BYTES)
    yield types.SimpleNamespace(K=K, L=K.lib(), rf=rf, ctx=rf._ctx.ptr, chunk=chunk)
    chunk.close()
    rf.close()


def stats(env):
    out = (C.c_uint64 * 6)()
    assert env.L.ts_bam_index_stats(env.ctx, out) == env.K.TS_OK
    return list(out)


def geometry(env, S, K):
    assert env.L.ts_bam_chunk_set_index_geometry(env.chunk.ptr, S, K) == env.K.TS_OK, env.L.ts_last_error(env.ctx)


def index(env, start, cap):
    """ts_bam_chunk_index as Chunk.walk calls ts_bam_chunk_walk: -> (records, next, error, error_off), and what lies behind
    the records taken must be as it was."""
    K, chunk = env.K, env.chunk
    arr = (K.BamRecord * (cap + 1))()
    C.memset(arr, 0xEE, C.sizeof(arr))
    n, nxt, err, eoff = C.c_uint64(7), C.c_uint64(7), C.c_int(7), C.c_uint64(7)
    rc = env.L.ts_bam_chunk_index(chunk.ptr, start, arr, cap, C.byref(n), C.byref(nxt), C.byref(err), C.byref(eoff))
    assert rc == K.TS_OK, env.L.ts_last_error(env.ctx)
    assert n.value <= cap
    recs = []
    for i in range(n.value):
        assert arr[i].reserved == 0
        recs.append((arr[i].off, arr[i].block_size, arr[i].seq_at, arr[i].l_seq))
    rest = bytes(arr)[n.value * C.sizeof(K.BamRecord):]
    assert rest == b"\xee" * len(rest), "the index wrote behind the records it reported"
    return recs, nxt.value, err.value, eoff.value


def check(env, plain, start, cap, S, K, what="", model=None):
    """The index at geometry (S, K) against the serial kernel, ref_walk and (unless model is False) the model, statistics too."""
    geometry(env, S, K)
    before = stats(env)
    got = index(env, start, cap)
    after = stats(env)
    exp = B.ref_walk(plain, start, cap)
    assert got[1:] == exp[1:], "%s: (next, error, error_off) %r, reference %r" % (what, got[1:], exp[1:])
    assert len(got[0]) == len(exp[0]), "%s: %d records, reference %d" % (what, len(got[0]), len(exp[0]))
    for i, (g, e) in enumerate(zip(got[0], exp[0])):
        assert g == e, "%s: record %d is %r, reference %r" % (what, i, g, e)
    assert env.chunk.walk(start, cap) == got, what
    d = [a - b for a, b in zip(after, before)]
    assert d[0] == 1 and d[1] == d[2] + d[3] and d[4] == len(got[0]), (what, d)
    if model is not False:
        st = (model or I.Model(plain)).index(start, cap, S, K)[4]
        assert d[1:4] == [st["entered"], st["hits"], st["settled"]], (what, d, st)
        spans = 0 if cap == 0 or len(plain) - start < 4 else (len(plain) - 1) // S - start // S + 1
        assert d[5] == spans * K * 16, (what, d)
        return got, st
    return got, None


def test_geometry_refuses_bad_values(env):
    L, K, ch = env.L, env.K, env.chunk.ptr
    for S, k in ((0, 4), (32, 4), (96, 4), (1 << 31, 4), (256, 0), (256, 9)):
        assert L.ts_bam_chunk_set_index_geometry(ch, S, k) == K.TS_ERR_INVALID_ARG, (S, k)
    assert L.ts_bam_chunk_set_index_geometry(None, 256, 4) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_index_stats(None, (C.c_uint64 * 6)()) == K.TS_ERR_INVALID_ARG
    for S, k in ((64, 1), (1 << 30, 8), (1 << 18, 4)):
        assert L.ts_bam_chunk_set_index_geometry(ch, S, k) == K.TS_OK


@pytest.mark.parametrize("S,K", I.GEOMETRIES)
def test_index_verdicts(env, S, K):
    for name, stream, cap, expected in B.verdict_cases():
        plain = env.chunk.fill_plain(stream)
        got, _ = check(env, plain, 0, cap, S, K, name)
        assert got == ([tuple(r) for r in expected[0]],) + tuple(expected[1:]), name


def test_index_small_spans_boundaries_long_records_and_tails(env):
    """S = 64 with records of 40-400 bytes (most records cross several spans), a record that starts on a span boundary, one
    longer than 100 spans with spans in which no record starts, an incomplete last record, three bytes left; `from` > 0 in
    mid-span; a table that fills inside a span and exactly at a span's first record."""
    for S in (64, 256):
        stream, facts = I.boundary_stream(S)
        plain = env.chunk.fill_plain(stream)
        model = I.Model(plain)
        table = B.ref_walk(plain, 0, BIG)[0]
        for K in (1, 4):
            got, st = check(env, plain, 0, BIG, S, K, "boundary stream", model)
            assert got[1] == facts["complete"] and st["settled"] <= 1
        mid = next(r[0] for r in table if r[0] % S not in (0, 1) and r[0] > S)
        check(env, plain, mid, BIG, S, 4, "from in mid-span", model)
        check(env, plain, facts["on_boundary"], BIG, S, 4, "from on a span boundary", model)
        first_of_span = next(i for i in range(2, len(table)) if table[i][0] // S != table[i - 1][0] // S)
        inside = next(i for i in range(2, len(table)) if table[i][0] // S == table[i - 1][0] // S)
        for cap in (first_of_span, first_of_span + 1, inside, inside + 1, 1, 0, len(table), len(table) - 1):
            got, _ = check(env, plain, 0, cap, S, 4, "cap %d" % cap, model)
            assert got[1] == (table[cap][0] if cap < len(table) else facts["complete"])
        complete = facts["complete"]
        for tail in (0, 1, 3, 4, 35, 36):
            plain = env.chunk.fill_plain(stream[:complete + tail])
            got, _ = check(env, plain, 0, BIG, S, 4, "a tail of %d bytes" % tail)
            assert got[1:] == (complete, 0, 0)
            check(env, plain, complete, 9, S, 1, "from at the tail of %d bytes" % tail)


def test_index_decoys(env):
    """Aux bytes that are whole valid records ahead of a span's true entry: K + 1 of them leave the true entry out of the K
    rows, and the span is settled by the serial rule exactly there; K - 1 of them leave it in.  Each decoy's chain is
    self-consistent and rejoins the true one; the table holds no decoy either way."""
    for K, n_decoys, settled in ((1, 2, 1), (4, 5, 1), (4, 3, 0)):
        stream, span, entry = I.decoy_stream(256, n_decoys)
        plain = env.chunk.fill_plain(stream)
        got, st = check(env, plain, 0, BIG, 256, K, "%d decoys, K = %d" % (n_decoys, K))
        assert st["settled"] == settled and st["settled_spans"] == [span] * settled
        offs = [r[0] for r in got[0]]
        assert entry in offs and not any(span * 256 < o < entry for o in offs)
        check(env, plain, 0, BIG, 256, 8, "%d decoys, K = 8" % n_decoys)
        check(env, plain, 0, BIG, 1024, K, "%d decoys in a larger span" % n_decoys)


def test_index_fuzz_and_reused_chunk(env):
    """300 of the seeded streams whose distribution tests/test_bam_chunk_reference_cpu.py pins, one after the other through
    the one chunk (each fill leaves the bytes of longer streams before it behind the chunk's end), each from a random record
    boundary with a random table size and at a geometry that changes with the seed."""
    for seed in range(300):
        stream, starts, kind = B.fuzz_stream(seed)
        gen = random.Random(seed + 2_000_003)
        start, cap = gen.choice(starts), gen.choice((0, 1, 2, gen.randrange(1, 70), 1000))
        S, K = I.GEOMETRIES[seed % len(I.GEOMETRIES)]
        try:
            plain = env.chunk.fill_plain(stream)
            check(env, plain, start, cap, S, K, "seed %d" % seed)
            if seed % 10 == 0:
                check(env, plain, 0, BIG, 64, 4, "seed %d, whole" % seed)
        except AssertionError:
            print("index fuzz: seed %d, kind %d, start %d, cap %d, S %d, K %d" % (seed, kind, start, cap, S, K))
            raise


def test_index_short_reads_need_no_serial_rule(env):
    """6 000 well-formed records of 150 bases at the default geometry and at spans of 4 KiB: every span's entry is a
    candidate row with 4 slots; the one span settled by the serial rule is that of the incomplete last record."""
    stream = I.short_read_stream(29, 6000)
    plain = env.chunk.fill_plain(stream[:-100])
    model = I.Model(plain)
    for S, K in ((1 << 18, 4), (4096, 4), (4096, 1)):
        got, st = check(env, plain, 0, BIG, S, K, "short reads, S = %d" % S, model)
        assert len(got[0]) == 5999 and got[2] == 0
        assert st["settled"] <= 1 or K == 1                           # (one slot: a single false candidate ahead of an entry costs a miss)
        assert st["entered"] == got[1] // S + 1                       # (every span holds a record's start)


def test_index_carry_through_a_long_stream(env):
    """carry_plan's stream through the chunk, carry_from = next of the index before: the concatenated tables are one walk of
    the whole stream.  (The model is not run on these chunks of several MiB: the serial kernel and ref_walk are.)"""
    chunk = env.chunk
    stream, fills = B.carry_plan(7)
    whole = B.ref_walk(stream, 0, 1 << 30)
    carry_from = chunk.size()
    base, fed, table = -carry_from, 0, []
    for i, (sizes, cap) in enumerate(fills):
        piece = stream[fed:fed + sum(sizes)]
        fed += len(piece)
        base += carry_from
        mirror = chunk.fill(piece, B.pack_members(piece, sizes), carry_from)
        (recs, carry_from, err, _), _ = check(env, mirror, 0, cap, 4096 if i % 2 else 1 << 18, 4, "fill %d" % i, model=False)
        assert err == 0
        table += [(off + base, bs, seq_at, lseq) for off, bs, seq_at, lseq in recs]
    while True:
        (recs, carry_from, err, _), _ = check(env, chunk.mirror, carry_from, 1 << 16, 4096, 4, "after the last fill", model=False)
        table += [(off + base, bs, seq_at, lseq) for off, bs, seq_at, lseq in recs]
        if not recs:
            break
    assert fed == len(stream) and base + carry_from == len(stream) and err == 0
    assert table == whole[0]


# =================================================================================================================== route
@pytest.fixture(scope="module")
def icli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / "bam_index_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bam_index_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


COUNTERS = re.compile(rb"bam index: calls (\d+) entered (\d+) hits (\d+) settled (\d+) records (\d+) row bytes (\d+)")


def three(icli, args, path):
    """--walk index, --walk serial and --host on one file: the same exit status and stdout; -> the index run."""
    runs = [subprocess.run([icli, "--bam-subset"] + how + args + [str(path)], stdin=subprocess.DEVNULL, capture_output=True, timeout=300)
            for how in (["--walk", "index"], ["--walk", "serial"], ["--host"])]
    idx, ser, host = runs
    assert idx.returncode == ser.returncode == host.returncode, [(r.returncode, r.stderr[-300:]) for r in runs]
    assert idx.stdout == ser.stdout == host.stdout
    if idx.returncode == 0:
        total = int(re.search(rb"kept \d+ of (\d+) records", idx.stderr).group(1))
        c = [int(x) for x in COUNTERS.search(idx.stderr).groups()]
        assert c[0] >= 1 and c[4] == total and c[1] == c[2] + c[3] and c[5] > 0, c          # the index produced every record
        assert [int(x) for x in COUNTERS.search(ser.stderr).groups()] == [0] * 6
    else:
        def message(r):
            return [ln for ln in r.stderr.splitlines() if ln.startswith(b"Error:")]
        assert message(idx) == message(ser) == message(host) and message(idx)
    return idx


def test_route_short_reads(icli, tmp_path):
    from tests.test_bam_subset import _kept_names, build_bam, gunzip_members
    rng = np.random.default_rng(31)
    reads = []
    for i in range(20000):
        n = int(rng.integers(100, 301))
        s = seqgen.random_dna(rng, n).tobytes().decode()
        if i % 50 == 0:
            s = ("TTAGGG" * 60)[:n]
        reads.append(("s%d" % i, s))
    header, _, bam = build_bam(reads, 60000)
    path = tmp_path / "short.bam"
    path.write_bytes(bam)
    r = three(icli, ["-l", "42"], path)
    assert r.returncode == 0, r.stderr[-300:]
    names = _kept_names(gunzip_members(r.stdout), header)
    assert len(names) >= 400 and {"s0", "s50"} <= set(names)
    c = [int(x) for x in COUNTERS.search(r.stderr).groups()]
    assert c[3] <= c[0], "well-formed short reads: at most the incomplete tail of each call is settled by the serial rule"


def test_route_large_records(icli, tmp_path):
    from tests.test_bam_subset import bgzf_fancy, build_bam, gunzip_members, make_reads
    gen = random.Random(5)
    rng = np.random.default_rng(123)
    reads = make_reads()
    big = bytearray(seqgen.random_dna(rng, 1_400_000).tobytes())
    t = seqgen.repeat_array("CCCTAA", 2000).tobytes()
    big[-len(t):] = t
    reads.insert(200, ("big_telomeric", big.decode()))
    reads.insert(300, ("big_plain", seqgen.random_dna(rng, 1_200_000).tobytes().decode()))
    header, records, _ = build_bam(reads, 60000)
    path = tmp_path / "fancy.bam"
    path.write_bytes(bgzf_fancy(header + b"".join(records), 30011, gen))
    r = three(icli, ["--bam-chunk-bytes", str(1 << 20), "--reads-per-batch", "97"], path)
    assert r.returncode == 0, r.stderr[-500:]
    plain = gunzip_members(r.stdout)
    assert plain[:len(header)] == header and records[200] in plain


def test_route_error_scenarios(icli, tmp_path):
    """Garbage and a missing EOF marker; the 70 mutated files of the host route's robustness test, every one through one
    process per route: per file the same verdict, the same bytes or the same message."""
    from tests.test_bam_subset import EOF_BLOCK, bgzf, build_bam, make_reads
    from tests.test_gpu_bam_device import mutation_files_70
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bgzf(b"NOTBAM" + b"\0" * 100, 60000))
    r = three(icli, [], bad)
    assert r.returncode != 0 and b"not a BAM" in r.stderr
    _, _, bam = build_bam(make_reads()[:8], 60000)
    noeof = tmp_path / "noeof.bam"
    noeof.write_bytes(bam[:-len(EOF_BLOCK)])
    r = three(icli, [], noeof)
    assert r.returncode == 0 and b"missing the BGZF EOF marker" in r.stderr
    files = mutation_files_70()
    verdicts = {}
    for route, how in (("index", ["--walk", "index"]), ("serial", ["--walk", "serial"]), ("host", ["--host"])):
        d = tmp_path / route
        d.mkdir()
        paths = []
        for i, data in enumerate(files):
            p = d / ("m%03d.bam" % i)
            p.write_bytes(data)
            paths.append(p)
        lst = d / "list.txt"
        lst.write_text("".join(str(p) + "\n" for p in paths))
        r = subprocess.run([icli, "--bam-subset-each", str(lst)] + how + ["-x", "0", "-l", "18"], capture_output=True, timeout=300)
        assert r.returncode == 0, (route, r.returncode, r.stderr[-500:])
        out = []
        for p in paths:
            ok, err, res = (p.parent / (p.name + ext) for ext in (".ok", ".err", ".out"))
            assert ok.exists() != err.exists(), (route, p.name)
            out.append(("ok", ok.read_text(), res.read_bytes()) if ok.exists() else ("err", err.read_text(), None))
        verdicts[route] = out
        calls = int(COUNTERS.search(r.stderr).group(1))
        assert (calls > 0) == (route == "index")
    assert verdicts["index"] == verdicts["serial"] == verdicts["host"]
    kinds = [v[0] for v in verdicts["index"]]
    assert kinds.count("ok") >= 5 and kinds.count("err") >= 20
