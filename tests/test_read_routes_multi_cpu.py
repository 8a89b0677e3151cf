"""What the read routes on several contexts need that can be checked without a GPU: the staging and commit entry points are
declared in include/teloscan.h with a comment that names the reference loops they stand in for, exported by libteloscan.so and
bound in teloscope_amd/_capi.py; the routes take a per-context figures argument; tests/cpp/read_routes_multi_cli.cpp builds with
warnings as errors and refuses to run without a device.  With a device the routes run in tests/test_gpu_read_routes_multi.py."""
import ctypes as C
import os
import re
import subprocess

from tests import harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["ts_chunk_stage_upload", "ts_chunk_stage_inflate", "ts_chunk_staged", "ts_chunk_commit"]


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "read_routes_multi_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def test_header_declares_and_library_exports_the_staging_calls():
    """Fails without the feature."""
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    section = hdr[:hdr.index("ts_chunk_stage_upload(")].rsplit("/* ----", 1)[1]
    assert "src/input.cpp:" in section and "src/bgzf.cpp:" in section          # the reference loops the calls stand in for
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert lib.ts_abi_version() == 4
    L = K.lib()
    assert L.ts_chunk_staged.restype is C.c_uint64 and len(L.ts_chunk_stage_inflate.argtypes) == 6
    # null chunks are refused, not dereferenced
    assert L.ts_chunk_stage_upload(None, None, 0, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_chunk_stage_inflate(None, None, 0, None, 0, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_chunk_commit(None, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_chunk_staged(None) == 0


def test_routes_take_per_context_figures_and_say_what_they_run_on():
    io = open(os.path.join(ROOT, "include", "teloscope_mi355x_io.hpp")).read()
    assert "Runs on the filter's first context" not in io
    assert "struct ReadRouteDeviceStats" in io
    for route in ("bamSubsetDevice", "fastqSubsetDevice"):
        signature = io[io.index("inline", io.index(route + "(const std::string &inFile") - 40):]
        signature = signature[:signature.index("{")]
        assert "std::vector<ReadRouteDeviceStats> *perDevice = nullptr)" in signature, route


def test_cli_builds_and_refuses_without_a_device(tmp_path):
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    cli = build_cli(tmp_path / "read_routes_multi_cli")
    r = subprocess.run([cli, "-x", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--fastq-subset" in r.stderr and "--bam-subset" in r.stderr
    r = subprocess.run([cli, "--bam-subset", "--walk", "sideways"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "serial|index" in r.stderr
    if K.lib().ts_device_count() > 0:
        return                                                   # (with a device: tests/test_gpu_read_routes_multi.py)
    for route in ("--device", "--host"):
        r = subprocess.run([cli, "--fastq-subset", route, "--devices", "0,0", H.golden_path("testFiles/fastq_subset.fq")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr and r.stdout == ""
