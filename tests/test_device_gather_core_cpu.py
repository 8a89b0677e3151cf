"""The per-lane copy of ts_gather_pieces_kernel and the splitter that makes its jobs (teloscope_amd/csrc/gather_core.h), compiled
for the host by g++ under ASan + UBSan (tests/cpp/device_gather_host.cpp) and driven lane by lane through an accessor that checks
every access.  The kernel compiles the same functions, so a lane that reads a word behind a piece — a device segment may end with
its allocation — or stores over a neighbour's byte is a failure here and not a fault, or a silent wrong base, on a GPU.  No GPU
needed.

The program's cases: every source misalignment 0..15 x every destination misalignment 0..15 x n in 0..80 as one job each; n in
{1023, 1024, 1025, slice - 1, slice, slice + 1, 3 slices + 7} at four misalignment pairs through the splitter; pieces of 0, 1,
slice - 1, slice, slice + 1 and 5 slices + 3 bytes at odd destination offsets.  Per piece it asserts that the destination bytes
equal the source's, 32 guard bytes either side are unchanged, every loaded word holds a byte of [src, src + n), every store lies
in [dst, dst + n) and no byte is stored twice; and of the jobs that they tile the piece in order, none longer than a slice,
every cut but the first on a 16-byte boundary of the destination."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")


@pytest.fixture(scope="module")
def host_gather(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_core")
    exe = str(d / "device_gather_host")
    src = os.path.join(ROOT, "tests", "cpp", "device_gather_host.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe], capture_output=True, timeout=600, env=env)
        if r.returncode == 0:
            break
    return r


def test_lanes_and_splitter_under_sanitizers(host_gather):
    r = host_gather
    assert r.returncode == 0 and not r.stderr, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    m = re.fullmatch(rb"ok (\d+) pieces (\d+) jobs\n", r.stdout)
    assert m, r.stdout
    # 16 x 16 x 81 single jobs, 7 sizes x 4 pairs through the splitter (the 5 that fit a slice also directly), 6 x 6 splitter cases
    assert int(m.group(1)) == 16 * 16 * 81 + 4 * (7 + 5) + 36
    assert int(m.group(2)) > int(m.group(1))


def test_kernel_and_host_program_share_one_source():
    """gather.hip holds no copy logic of its own: it calls gather_core.h's copy_lane, the pipeline calls its splitter, and the
    build knows both files."""
    kernel = open(os.path.join(CSRC, "gather.hip")).read()
    assert '#include "gather_core.h"' in kernel and "tsgather::copy_lane(" in kernel and "asm" not in kernel
    assert "__shared__" not in kernel
    pipeline = open(os.path.join(CSRC, "pipeline.cpp")).read()
    assert "tsgather::split_piece(" in pipeline and "ts_k_launch_gather_pieces(" in pipeline
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\bgather\.hip\b", mk, re.M) and re.search(r"^HDRS\s*:=.*gather_core\.h\b", mk, re.M)


def test_stats_entry_point_is_declared_and_bound():
    """ts_device_input_stats: in the header (ABI 4 still), in the ctypes list with its argument types, in the C++ mirror and on
    the Python class."""
    from teloscope_amd import _capi as K
    import teloscope_amd as ta
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    assert re.search(r"int\s+ts_device_input_stats\(const ts_ctx \*ctx, uint64_t out\[4\]\);", hdr)
    assert "ts_device_input_stats" in K.SYMBOLS and K.lib().ts_device_input_stats.argtypes is not None
    assert K.lib().ts_abi_version() == 4
    assert "deviceInputStats()" in open(os.path.join(ROOT, "include", "teloscope_mi355x.hpp")).read()
    assert callable(ta.Teloscope.device_input_stats)
    assert K.lib().ts_device_input_stats(None, None) == K.TS_ERR_INVALID_ARG
    from teloscope_amd.cli import parse_cli, user_input
    tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=K.DEVICE_NONE))      # (planning-only: nothing seen, ever)
    assert tel.device_input_stats() == (0, 0, 0, 0)
    tel.close()
