"""Without a device: the plain-Python GFA references of tests/gfachunk.py (what tests/test_gpu_gfa_chunk.py holds the device stage
against) pinned by the host reader — tests/cpp/gfa_device_cli.cpp --dump-records prints readGfa's view of a file — on every
committed GFA input, on the generators' edge cases and on all of them again with CRLF line ends; the C-ABI of the device stage
declared and exported, its structs mirrored; the test program builds and refuses to run without a device."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from tests import gfachunk as G
from tests import harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = sorted(glob.glob(os.path.join(H.GOLDEN, "testFiles", "*.gfa")))
NEW_ENTRY_POINTS = ["ts_gfa_chunk_walk", "ts_chunk_data", "ts_chunk_carry_over"]


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gfa_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("gfa_cli") / "gfa_device_cli")


def host_dump(cli, path):
    r = subprocess.run([cli, "--dump-records", str(path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def check(cli, tmp_path, text, what):
    for tag, t in (("lf", text), ("crlf", G.crlf(text))):
        path = tmp_path / ("case.%s.gfa" % tag)
        path.write_bytes(t)
        assert G.ref_dump(t, path) == host_dump(cli, path), "%s (%s)" % (what, tag)


def test_inputs_are_there():
    assert len(INPUTS) == 16


@pytest.mark.parametrize("path", INPUTS, ids=lambda p: os.path.basename(p))
def test_reference_equals_host_reader_on_committed_graphs(cli, tmp_path, path):
    text = open(path, "rb").read()
    assert G.ref_dump(text, path) == host_dump(cli, path)
    check(cli, tmp_path, text, os.path.basename(path))
    # the same tables from a text cut anywhere: what is not consumed is carried
    whole = G.ref_walk(text, True)
    for cut in range(0, len(text), max(1, len(text) // 23)):
        s1, l1, t1, nxt, f1 = G.ref_walk(text[:cut], False)
        s2, l2, t2, nxt2, f2 = G.ref_walk(text[nxt:], True)
        assert nxt <= cut and nxt + nxt2 == len(text)
        assert [s[:9] for s in s1] + [(s[0] + nxt,) + s[1:9] for s in s2] == [s[:9] for s in whole[0]]
        assert [l[:3] for l in l1] + [(l[0] + nxt,) + l[1:3] for l in l2] == [l[:3] for l in whole[1]]
        assert t1 + t2 == whole[2]
        assert (f1 if f1 is not None else (None if f2 is None else (f2[0] + nxt, f2[1]))) == whole[4]


@pytest.mark.parametrize("name", sorted(G.edge_cases()))
def test_reference_equals_host_reader_on_edge_cases(cli, tmp_path, name):
    check(cli, tmp_path, G.edge_cases()[name], name)


def test_edge_cases_hold_what_they_name(tmp_path):
    e = G.edge_cases()
    graph = lambda k: G.ref_graph(e[k], "x.gfa")
    walk = lambda k: G.ref_walk(e[k], True)
    assert walk("empty") == ([], [], b"", 0, None) and walk("only blank lines")[:3] == ([], [], b"")
    assert [s[2] for s in walk("S with nine tabs")[0]] == [5, 5] and len(walk("S alone")[0]) == 3 and len(walk("S with two fields")[0]) == 3
    assert [s for _, s in graph("S with a star")["segments"]][0::2] == [None, None]
    assert [s for _, s in graph("S with an empty sequence")["segments"]][0::2] == [b"", b""]
    assert graph("empty name")["segments"][0][0] == b""
    assert walk("SX is not single")[4] == (0, 2) and len(walk("SX is not single")[0]) == 3
    g = graph("gfa2 with and without tags")
    assert g["version"] == 2 and [len(s) for _, s in g["segments"]] == [400, 333] and len(g["edits"]) == 3
    assert [None if s is None else len(s) for _, s in graph("gfa2 with three fields only")["segments"]] == [400, None, 90]
    assert [s for _, s in graph("gfa2 stars")["segments"]][:2] == [None, None] and graph("gfa2 stars")["segments"][3][1] is None
    g = graph("gfa2 header as the last line")
    assert g["version"] == 2 and [len(s) for _, s in g["segments"]] == [400, 333]
    assert graph("two headers, 2.0 then 1.1")["version"] == 1 and graph("two headers, 2.0 then 1.1")["edits"][0][2] == b"H\tVN:Z:1.2"
    assert graph("two headers, 1.0 then 2.0")["version"] == 2
    assert graph("header without VN")["has_version"] is False and len(walk("header without VN")[1]) == 2
    assert [len(c) for _, c in graph("paths before their segments")["paths"]] == [2, 1]
    assert graph("path with semicolons")["paths"][0][1] == [(b"a", b"+"), (b"b", b"+"), (b"c", b"-")]
    assert graph("path components without orientation")["paths"][0][1] == [(b"b", b"+"), (b"c", b"x"), (b"c", b"+")]
    assert [n for n, _ in graph("path lines that are no paths")["paths"]] == [b"ok"] and len(walk("path lines that are no paths")[1]) == 3
    assert b"segment 'b' is defined twice" in graph("duplicate segment name")["error"]
    assert b"record type 'E'" in graph("gfa2 with an E record")["error"]
    assert b"record type 'GG'" in graph("gfa2 whose first foreign line is not its first")["error"]
    assert b"record type 'E'" in graph("gfa2 with a foreign first line")["error"]
    assert walk("L, W and C lines in a gfa1 input")[4][1] == 1 and "error" not in graph("L, W and C lines in a gfa1 input")
    assert graph("pathless graph")["paths"] == [] and walk("comment lines")[4] is None
    # the unfinished last line is the carry; with at_end it is a line, and a '\r' at its end is no content
    assert G.ref_walk(b"S\ta\tAC\nS\tb\tGG", False)[3] == 7 and len(G.ref_walk(b"S\ta\tAC\nS\tb\tGG", False)[0]) == 1
    assert G.ref_walk(b"S\ta\tAC\nS\tb\tGG\r", True)[0][1][6] == 2 and G.ref_walk(b"S\ta\tAC", False)[3] == 0
    for seed, text in ((1, G.pathless_graph(1, 40)), (2, G.path_graph(2, 60, 6)), (3, G.mixed_lines(3, 500))):
        assert "error" not in G.ref_graph(text, "x.gfa"), seed


def test_generated_graphs_equal_host_reader(cli, tmp_path):
    for what, text in (("pathless", G.pathless_graph(1, 40)), ("paths", G.path_graph(2, 60, 6)), ("mixed", G.mixed_lines(3, 500))):
        check(cli, tmp_path, text, what)


def test_header_declares_and_library_exports_the_device_stage():
    """Fails without the feature: include/teloscan.h declares the GFA stage, libteloscan.so exports it, and the ABI version has
    not moved."""
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    assert "src/input.cpp:" in hdr[hdr.index("GFA text in the same resident chunk"):hdr.index("typedef struct ts_gfa_segment")]
    assert re.search(r"#define\s+TELOSCAN_ABI_VERSION\s+4\b", bare)
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert lib.ts_abi_version() == 4
    assert (C.sizeof(K.GfaSegment), C.sizeof(K.GfaLine), C.sizeof(K.GfaForeign)) == (48, 24, 16)


def test_struct_mirrors_match_the_c_structs(tmp_path):
    from teloscope_amd import _capi as K
    fields = {"ts_gfa_segment": (K.GfaSegment, ["off", "len", "n_fields", "f1_at", "f1_len", "f2_at", "f2_len", "f3_at", "f3_len", "name_at", "star"]),
              "ts_gfa_line": (K.GfaLine, ["off", "len", "kind", "text_at", "reserved"]),
              "ts_gfa_foreign": (K.GfaForeign, ["off", "len", "found"])}
    body = "".join('printf("%%zu ", sizeof(%s));%s' % (t, "".join('printf("%%zu ", offsetof(%s, %s));' % (t, f) for f in fs))
                   for t, (_, fs) in sorted(fields.items()))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "teloscan.h"\nint main(void){%s return 0;}' % body)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for t, (R, fs) in sorted(fields.items()):
        want += [C.sizeof(R)] + [getattr(R, f).offset for f in fs]
    assert got == want


def test_cli_refuses_without_a_device(cli):
    from teloscope_amd import _capi as K
    r = subprocess.run([cli, "-t", "1000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--device" in r.stderr and "--dump-records" in r.stderr
    if K.lib().ts_device_count() > 0:
        return                                                   # (with a device: tests/test_gpu_gfa_device.py)
    for route in ("--device", "--host"):
        r = subprocess.run([cli, route, "-f", H.golden_path("testFiles/gfa_telo.gfa")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr and r.stdout == ""
