"""The parallel record index (ts_bam_chunk_index) where no device is needed: the plain-Python model of its scheme
(tests/bamindex.py: spans, candidates, chain, write) against ref_walk, the condition that well-formed input never needs the
serial rule except for the chunk's incomplete tail, and teloscope_amd/csrc/bam_walk_core.h — the code the kernels compile — run
by a program of its own under ASan + UBSan (tests/cpp/bam_index_host.cpp) against the model, tables and statistics alike.
tests/test_gpu_bam_index.py holds the kernels to the same model."""
import os
import re
import subprocess

import pytest

from tests import bamchunk as B
from tests import bamindex as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
BIG = 1 << 30


def check(model, start, cap, S, K):
    got = model.index(start, cap, S, K)
    assert got[:4] == B.ref_walk(model.plain, start, cap), (start, cap, S, K)
    st = got[4]
    assert st["entered"] == st["hits"] + st["settled"]
    return got


@pytest.mark.parametrize("S,K", I.GEOMETRIES)
def test_model_equals_ref_walk_on_hand_written_streams(S, K):
    for name, stream, cap, expected in B.verdict_cases():
        got = check(I.Model(stream), 0, cap, S, K)
        assert got[:4] == expected, name


@pytest.fixture(scope="module")
def fuzz_models():
    return [(I.Model(B.fuzz_stream(seed)[0]), seed % 6) for seed in range(B.FUZZ_SEEDS)]


@pytest.mark.parametrize("S,K", I.GEOMETRIES)
def test_model_equals_ref_walk_on_the_fuzz_streams(fuzz_models, S, K):
    for seed, (model, kind) in enumerate(fuzz_models):
        st = check(model, 0, BIG, S, K)[4]
        if kind in (1, 2, 3, 4):                                    # the span of the mutated record misses, as it must
            assert st["settled"] >= 1, seed
        if seed % 7 == 0:                                           # a start in mid-stream and a table that fills
            table = B.ref_walk(model.plain, 0, BIG)[0]
            if len(table) > 3:
                check(model, table[2][0], len(table) - 3, S, K)
                check(model, table[1][0], 1, S, K)


@pytest.mark.parametrize("S,K", I.GEOMETRIES)
def test_model_equals_ref_walk_on_the_placement_streams(S, K):
    for first in (0, 8192, 8193, 40000):
        for d in (0, 1, 150, 291, 292, 300):
            stream, at = B.placement_stream(1000 * d + first, first, d)
            model = I.Model(stream)
            st = check(model, 0, BIG, S, K)[4]
            assert st["settled"] == 0
            check(model, at, BIG, S, K)
            check(model, 0, 5, S, K)


def well_formed_inputs():
    for seed in range(B.FUZZ_SEEDS):
        if seed % 6 in (0, 5):
            yield "fuzz %d" % seed, B.fuzz_stream(seed)[0]
    yield "short reads", I.short_read_stream(17, 3000)


def test_well_formed_input_needs_the_serial_rule_only_for_the_incomplete_tail():
    """A condition, not a measurement: on well-formed records (fuzz kinds 0 and 5; 3 000 records of 150 bases with random SEQ,
    qualities 2 .. 40 and mapped positions) no span's true entry is missing from its first 4 candidates, at any span size.
    The one span that may be settled by the serial rule is the one whose entry is the chunk's incomplete last record."""
    for name, stream in well_formed_inputs():
        model = I.Model(stream)
        for S in (64, 256, 1024, 4096, 65536):
            table, nxt, err, _, st = check(model, 0, BIG, S, 4)
            assert err == 0
            if st["settled"]:
                assert st["settled"] == 1 and nxt // S == st["settled_spans"][0], (name, S, st)
                assert I.record_at(model.plain, nxt)[0] in (I.INCOMPLETE, I.SHORT), (name, S)


def test_decoys_fill_the_slots_exactly_where_the_model_says():
    for K, n_decoys, settled in ((1, 2, [3]), (4, 5, [3]), (4, 3, [])):
        stream, span, entry = I.decoy_stream(256, n_decoys)
        model = I.Model(stream)
        rows = model.rows(span, 256, K, 0)
        assert len(rows) == K and [r[0] for r in rows][:n_decoys] == [3 * 256 + 2 + 40 * i for i in range(min(K, n_decoys))]
        assert (entry in [r[0] for r in rows]) == (not settled)
        st = check(model, 0, BIG, 256, K)[4]
        assert st["settled_spans"] == settled
        assert entry in [r[0] for r in B.ref_walk(stream, 0, BIG)[0]]
        assert not any(3 * 256 < r[0] < entry for r in B.ref_walk(stream, 0, BIG)[0])      # no decoy in the table


def test_boundary_stream_holds_what_it_says():
    for S in (64, 256):
        stream, facts = I.boundary_stream(S)
        table, nxt, err, _ = B.ref_walk(stream, 0, BIG)
        offs = [r[0] for r in table]
        assert facts["on_boundary"] in offs and facts["on_boundary"] % S == 0
        assert table[offs.index(facts["long_at"])][1] + 4 > 100 * S
        assert (nxt, err) == (facts["complete"], 0) and 4 <= len(stream) - nxt
        starts = {o // S for o in offs}
        assert any(k not in starts for k in range(facts["long_at"] // S + 1, facts["long_at"] // S + 100))
        for K in (1, 4):
            check(I.Model(stream), 0, BIG, S, K)


# ------------------------------------------------------------------------------------------------ the core under sanitizers
@pytest.fixture(scope="module")
def host_index(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_index")
    exe = str(d / "bam_index_host")
    src = os.path.join(ROOT, "tests", "cpp", "bam_index_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    empty = str(d / "empty.bin")
    open(empty, "wb").close()
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        if subprocess.run([exe, empty], capture_output=True, timeout=60, env=ENV).returncode == 0:
            break
    return exe, d


def host_cases():
    """[(stream, from, cap, S, K)]: every hand-written stream at every geometry, the fuzz streams at three, placement, decoy,
    boundary and short-read streams, starts in mid-span and tables that fill inside a span and at its first record."""
    cases = []
    for _, stream, cap, _ in B.verdict_cases():
        cases += [(stream, 0, cap, S, K) for S, K in I.GEOMETRIES]
    for seed in range(B.FUZZ_SEEDS):
        stream = B.fuzz_stream(seed)[0]
        cases += [(stream, 0, BIG, 64, 1), (stream, 0, BIG, 1024, 4)]
        if seed % 5 == 0:
            table = B.ref_walk(stream, 0, BIG)[0]
            cases.append((stream, table[len(table) // 2][0] if table else 0, max(1, len(table) // 3), 256, 4))
    for first, d in ((0, 0), (0, 291), (8193, 100), (40000, 292)):
        stream = B.placement_stream(1000 * d + first, first, d)[0]
        cases += [(stream, 0, BIG, 256, 4), (stream, 0, 7, 1024, 1)]
    for K, n_decoys in ((1, 2), (4, 5), (4, 3)):
        cases.append((I.decoy_stream(256, n_decoys)[0], 0, BIG, 256, K))
    for S in (64, 256):
        stream = I.boundary_stream(S)[0]
        cases += [(stream, 0, BIG, S, 4), (stream, 0, BIG, S, 1)]
    reads = I.short_read_stream(3, 400)
    table = B.ref_walk(reads, 0, BIG)[0]
    at_span_start = next(i for i in range(1, len(table)) if table[i][0] // 1024 != table[i - 1][0] // 1024)
    cases += [(reads, 0, BIG, 1024, 4), (reads, table[5][0], BIG, 4096, 4), (reads, 0, at_span_start, 1024, 4),
              (reads, 0, at_span_start + 1, 1024, 4), (reads, 0, 0, 64, 4), (reads, len(reads), 9, 64, 4), (reads[:-3], len(reads) - 6, 9, 64, 4)]
    return cases


def test_core_equals_the_model_under_sanitizers(host_index):
    exe, d = host_index
    cases = host_cases()
    path = str(d / "cases.bin")
    I.case_file(path, cases)
    r = subprocess.run([exe, path], capture_output=True, timeout=900, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    models = {}
    for i, (line, (stream, start, cap, S, K)) in enumerate(zip(lines, cases)):
        model = models.get(id(stream)) or models.setdefault(id(stream), I.Model(stream))
        want = model.index(start, cap, S, K)
        assert want[:4] == B.ref_walk(stream, start, cap)
        assert line == I.result_line(want), (i, start, cap, S, K)


def test_entry_points_are_declared_exported_and_documented():
    """Fails without the feature: the three entry points in the header (each citing the reference interface it replaces), in
    the Python symbol list and in the library; the mirror's walk selector."""
    import ctypes as C

    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    assert re.search(r"int ts_bam_chunk_index\(ts_bam_chunk \*chunk, uint64_t from, ts_bam_record \*recs, uint64_t cap, uint64_t \*n, uint64_t \*next,\s*"
                     r"int \*error, uint64_t \*error_off\);", hdr)
    assert "int ts_bam_chunk_set_index_geometry(ts_bam_chunk *chunk, uint32_t span_bytes, uint32_t candidates);" in hdr
    assert "int ts_bam_index_stats(const ts_ctx *ctx, uint64_t out[6]);" in hdr
    for name in ("ts_bam_chunk_index", "ts_bam_chunk_set_index_geometry", "ts_bam_index_stats"):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "src/bam.cpp:188-259" in comment, name
        assert name in K.SYMBOLS
        assert hasattr(C.CDLL(K.LIB_PATH), name), name
    mirror = open(os.path.join(ROOT, "include", "teloscope_mi355x_io.hpp")).read()
    assert "enum class BamRecordWalk" in mirror and "BamRecordWalk walk" in mirror


def test_kernels_and_host_program_share_one_source():
    kernels = open(os.path.join(CSRC, "bgzf.hip")).read()
    assert '#include "bam_walk_core.h"' in kernels
    for use in ("tsbam::candidate(", "tsbam::span_walk(", "tsbam::scan_range("):
        assert use in kernels, use
    serial = kernels[kernels.index("void ts_bam_walk_kernel("):kernels.index("// ---- the parallel record index")]
    assert "tsbam::" not in serial, "the serial walk stays an independent statement of the rule"
    assert "tsbam::chain(" in open(os.path.join(CSRC, "bgzf.cpp")).read()
    host = open(os.path.join(ROOT, "tests", "cpp", "bam_index_host.cpp")).read()
    assert "teloscope_amd/csrc/bam_walk_core.h" in host and "tsbam::chain(" in host and "tsbam::candidate(" in host
