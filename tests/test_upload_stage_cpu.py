"""The layer between the packing primitives and the DMA of the host upload (teloscope_amd/csrc/upload_stage_core.h): which pieces
make a chunk, what the staging workers write into its slot on the packed and on the ASCII route, the tail of a packed chunk and
its ts_upload_stats increments — compiled for the host by g++ under ASan + UBSan together with a program of its own
(tests/cpp/upload_stage_host.cpp) and compared there with a statement made a position at a time; the pooled cases a second time
under TSan, with StagePool's threads over one shared slot.  Every source and every destination is a heap block of exactly the
size the contract allows.  No GPU needed, nothing loaded into Python is under a sanitizer.

What the program pins beyond equality is said at its top; this file asks that the cases reached every decision, restates the two
rules of a chunk's extent, and checks that the driver (pipeline.cpp: upload_pieces) kept none of the logic for itself."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "upload_stage_host.cpp"), os.path.join(CSRC, "pack.cpp")]
PACKED_CASES = 640
SEED = 20261021


def fields(line):
    words = line.split()
    return {k: int(v) for k, v in zip(words[1::2], words[2::2])}


def usage_answer(out):
    r = subprocess.run([out], capture_output=True)
    return r.returncode == 2 and b"usage" in r.stderr, r.stderr.decode(errors="replace")[-2000:]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("upload_stage") / "upload_stage_host")
    base = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + SOURCES + ["-pthread", "-o", out]
    for more in ([], ["-static-libasan"]):                         # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + more)
        ok, err = usage_answer(out)
        if ok:
            break
    assert ok, err
    return out


@pytest.fixture(scope="module")
def exe_tsan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("upload_stage_tsan") / "upload_stage_host")
    base = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread"] + SOURCES + ["-pthread", "-o", out]
    why = ""
    for more in ([], ["-static-libtsan"]):
        r = subprocess.run(base + more, capture_output=True)
        if r.returncode != 0:
            why = r.stderr.decode(errors="replace")
            assert "tsan" in why.lower(), why[-3000:]              # (anything else is an error of the program's)
            continue
        ok, why = usage_answer(out)
        if ok:
            return out
    pytest.skip("this toolchain has no usable ThreadSanitizer runtime: " + why.strip()[-300:])


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, timeout=1200, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    return r.stdout.decode()


def reached_every_decision(out):
    for kind in ("plain", "text", "copied", "mixed"):
        assert out[kind] > 0, kind
    for phase in range(4):                                          # (d0 ^ i0) & 3 of copied codes
        assert out["phase%d" % phase] > 0, phase
    for a in range(3):                                              # plain, text, packed: every ordered pair meets inside a block
        for b in range(3):
            assert out["seam%d%d" % (a, b)] > 0, (a, b)
    for what in ("short_text", "n_over_block", "n_over_cut", "merged_runs", "several_workers", "off_boundary", "ends_on_block", "ends_on_cut"):
        assert out[what] > 0, what


def test_packed_chunks_one_worker_after_the_other(exe):
    """Chunks of 1 to 5 x 16384 + 63 positions from every first-base offset within 64, of plain, text and packed pieces and of all
    three, each staged by 1 to 8 workers that are handed exactly their bytes of the slot.  (In parallel parts: one process would
    take a quarter of a minute under the sanitizers.)"""
    parts = max(1, min(8, len(os.sched_getaffinity(0))))
    procs = [subprocess.Popen([exe, "packed", str(SEED), str(PACKED_CASES), str(p), str(parts)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV)
             for p in range(parts)]
    total = {}
    for p in procs:
        out, err = p.communicate(timeout=1200)
        assert p.returncode == 0 and not err, err.decode(errors="replace")[-3000:]
        for k, v in fields(out.decode()).items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert total["chunks"] == 8 * PACKED_CASES
    reached_every_decision(total)


def test_packed_chunks_pooled(exe):
    """The same chunks with StagePool's threads writing one shared slot of exactly packed_bytes(P) + 8 bytes."""
    out = fields(run([exe, "pooled", str(SEED), "160"]))
    assert out["chunks"] == 8 * 160 and out["several_workers"] > 0


def test_ascii_chunks(exe):
    """The ASCII route's three forms — one worker, whole pieces handed out dynamically, equal byte shares of plain pieces — into a
    block of exactly the chunk's bytes: the pieces' bases as they lie at the source, nothing between them written, short text
    reported."""
    out = fields(run([exe, "ascii", str(SEED), "90"]))
    assert out["single"] == 90 and out["whole_pieces"] == 8 * 90 and out["shares"] == 8 * 45 and out["short_text"] > 0


def test_pooled_cases_under_thread_sanitizer(exe_tsan):
    out = fields(run([exe_tsan, "pooled", str(SEED), "60"]))
    assert out["chunks"] == 8 * 60 and out["several_workers"] > 0
    out = fields(run([exe_tsan, "ascii", str(SEED), "30"]))
    assert out["whole_pieces"] == 8 * 30 and out["shares"] == 8 * 15


def test_call_pieces(exe):
    """Device pieces set aside, plain and packed pieces cut at the limit (sources and first codes advanced), a text piece at the
    limit taken whole and one over it refused."""
    assert fields(run([exe, "normalise"]))["ok"] == 1


def test_chunk_extent_against_the_two_rules(exe):
    """A chunk takes the next piece while the span from its first base to that piece's end is at most the limit and the piece
    begins at most the gap behind the end of the one before it; the first piece is taken whatever its length."""
    lines = run([exe, "extent", str(SEED), "2000"]).splitlines()
    assert len(lines) == 2000
    several = at_limit = at_gap = 0
    for line in lines:
        head, chunks = line.split(" chunks ")
        head, pieces = head.split(" pieces ")
        limit, gap = (int(w) for w in head.split()[1::2])
        nums = [int(w) for w in pieces.split()]
        pieces = list(zip(nums[0::2], nums[1::2]))
        nums = [int(w) for w in chunks.split()]
        got = list(zip(nums[0::2], nums[1::2]))
        want, i = [], 0
        while i < len(pieces):
            j, total = i + 1, pieces[i][1]
            while j < len(pieces) and sum(pieces[j]) - pieces[i][0] <= limit and pieces[j][0] - sum(pieces[j - 1]) <= gap:
                total += pieces[j][1]
                j += 1
            several += j - i > 1
            at_limit += j - i > 1 and sum(pieces[j - 1]) - pieces[i][0] == limit
            at_gap += j - i > 1 and any(pieces[k][0] - sum(pieces[k - 1]) == gap for k in range(i + 1, j))
            want.append((j, total))
            i = j
        assert got == want, line
    assert several > 500 and at_limit > 20 and at_gap > 100, (several, at_limit, at_gap)


def test_driver_keeps_none_of_the_staging_logic():
    """pipeline.cpp drives: slots, DMAs, launches, counters.  The 2-bit arithmetic, the thread pool and the walk over a chunk's
    blocks live in the header that the host program tests, and that header needs no device."""
    text = open(os.path.join(CSRC, "pipeline.cpp")).read()
    assert '#include "upload_stage_core.h"' in text
    assert "struct StagePool" not in text and "struct UpPiece" not in text
    assert not re.search(r">>\s*\(2u?\s*\*", text) and not re.search(r"<<\s*\(2u?\s*\*", text) and '"ACTG"' not in text      # the 2-bit extract / deposit
    body = text[text.index("int upload_pieces("):text.index("int region_pieces(")]
    assert "16384" not in body and "BK" not in body and "kBlock" not in body and "pack_bases" not in body and "pack_text" not in body
    for use in ("tsstage::normalise_pieces(", "tsstage::chunk_extent(", "tsstage::PackedChunk", "tsstage::ascii_single(", "tsstage::ascii_whole_pieces(",
                "tsstage::ascii_share(", "tsstage::StagePool"):
        assert use in body, use
    assert body.count("hipEventRecord(") == 1 and body.count("ts_ctx::kUpSlots") == 2          # the slot advance, written once (and the allocation loop)
    core = open(os.path.join(CSRC, "upload_stage_core.h")).read()
    assert re.findall(r'#include "([^"]+)"', core) == ["host.hpp", "text_core.h"] and "hip_runtime" not in core and "ts_ctx *" not in core
    host = open(os.path.join(ROOT, "tests", "cpp", "upload_stage_host.cpp")).read()
    assert "teloscope_amd/csrc/upload_stage_core.h" in host
