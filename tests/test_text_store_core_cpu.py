"""The store plan of the device text formatters (teloscope_amd/csrc/text_store_core.h) on the host: how a wave's staged text is
cut into head bytes, aligned 16-byte pieces and tail bytes, compiled by g++ under ASan + UBSan as a program of its own
(tests/cpp/text_store_host.cpp) that plays the 64 lanes — the gfx950 kernels of tracks.hip and match_text.hip take the same
numbers from the same header, through ts_text_emit.h.  A second build with a seeded fault has to fail.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def build_and_run(d, name, defines=()):
    exe = str(d / name)
    src = os.path.join(ROOT, "tests", "cpp", "text_store_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *defines, src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe], capture_output=True, timeout=120, env=ENV)
        if r.returncode == 0 or b"checks failed" in r.stderr:       # (the program ran: its verdict stands)
            break
    return r


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("text_store")


def test_every_byte_once_aligned_and_in_bounds_under_sanitizers(build_dir):
    r = build_and_run(build_dir, "text_store_host")
    assert r.returncode == 0 and not r.stderr, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    m = re.fullmatch(rb"ok (\d+) cases\n", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == 2 * 16 * (601 + 17)                   # two bases, every shift, n in 0..600 and 8176..8192


def test_the_seeded_fault_is_found(build_dir):
    """v0 computed as shift / 16: wherever the staged text is shifted and has a body, the 16-byte pieces come from one vector
    too early — the program has to say so."""
    r = build_and_run(build_dir, "text_store_host_fault", ["-DSEED_V0_FAULT"])
    assert r.returncode == 1 and b"arrived as" in r.stderr and b"checks failed" in r.stderr, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert b"shift 0:" not in r.stderr                              # (an unshifted destination reads vector 0 either way)


def test_both_formatters_take_the_plan_from_the_core():
    emit = open(os.path.join(CSRC, "ts_text_emit.h")).read()
    assert '#include "text_store_core.h"' in emit and "tsstore::plan(" in emit and "tsstore::staged(" in emit
    for kernel in ("tracks.hip", "match_text.hip"):
        text = open(os.path.join(CSRC, kernel)).read()
        assert '#include "ts_text_emit.h"' in text and "wave_put(" in text and "wave_copy_out(" in text
        for own in ("struct StageSink", "struct GlobalSink", "& 15u", "kStageBytes"):      # no copy of the sinks or the arithmetic
            assert own not in text, (kernel, own)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HDRS\s*:=.*text_store_core\.h\b.*ts_text_emit\.h\b", mk, re.M)
