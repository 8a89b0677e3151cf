"""Without a device: the plain-Python SAM walk of tests/samchunk.py (what tests/test_gpu_sam_chunk.py holds the device walk
against) pinned against the host route's walk (tests/cpp/sam_device_cli.cpp --dump-records: detail::samWalkHost of
include/teloscope_mi355x_io.hpp) and against the per-line rule the kernels compile (teloscope_amd/csrc/sam_line_core.h through
tests/cpp/sam_line_host.cpp, a stand-alone program under ASan + UBSan) on every generated case, with LF and with CR LF line ends;
the C-ABI of the device route declared and exported; the test program builds and refuses to run a route without a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import harness as H
from tests import samchunk as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["ts_sam_chunk_walk", "ts_sam_chunk_stage", "ts_sam_chunk_gather"]


def all_cases():
    """name -> complete text: every edge and error case as it is and, where it holds no '\\r' yet, with CR LF line ends."""
    cases = dict(S.edge_cases())
    cases.update({name: text for name, (text, _, _) in S.error_cases().items()})
    for name, text in list(cases.items()):
        if b"\r" not in text:
            cases[name + " (crlf)"] = text.replace(b"\n", b"\r\n")
    return cases


CASES = all_cases()


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sam_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(sam_device_cli, sam_line_host under ASan + UBSan, a directory with every case as a file)"""
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    d = tmp_path_factory.mktemp("sam_cpu")
    cli = build_cli(d / "sam_device_cli")
    host = str(d / "sam_line_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "sam_line_host.cpp"), "-o", host])
    files = {}
    for i, (name, text) in enumerate(sorted(CASES.items())):
        files[name] = d / ("case%03d.sam" % i)
        files[name].write_bytes(text)
    return cli, host, files


def parse_dump(stdout):
    recs, head, tail = [], None, None
    for line in stdout.decode().splitlines():
        w = line.split()
        if w[0] == "header":
            head = (int(w[1]), int(w[2]))
        elif w[0] == "record":
            recs.append(tuple(int(x) for x in w[1:]))
        else:
            assert w[0] == "lines" and w[2] == "next" and w[4] == "error"
            tail = (int(w[1]), int(w[3]), int(w[5]), int(w[6]), int(w[7]))
    return (recs,) + head + tail


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_walk_equals_the_host_walk(programs, name):
    cli, _, files = programs
    assert dump(cli, files[name]) == S.ref_walk(CASES[name], True, True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_line_rule_under_sanitizers_equals_the_reference(programs, name):
    """The rule the kernels compile, a line at a time over a line index and a tab index made as the chunk layer makes them, in
    heap blocks of the exact sizes: kind, error and, for a valid line, the record, for every whole line under both at_end."""
    _, host, files = programs
    text = CASES[name]
    for at_end in (1, 0):
        r = subprocess.run([host, str(files[name]), str(at_end)], capture_output=True, timeout=60)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = [l.split() for l in r.stdout.decode().splitlines()]
        lines = S.lines_of(text, bool(at_end))
        assert len(got) == len(lines)
        for g, (b, e, line_end, _) in zip(got, lines):
            if text[b:b + 1] == b"@":
                assert g == ["H", str(b)]
                continue
            err, rec = S.ref_line(text, b, e, line_end)
            assert g[:3] == ["A", str(b), str(err)], (g, b, err)
            if err == S.OK:
                assert tuple(int(x) for x in g[3:]) == rec[1:], (g, rec)


def dump(cli, path):
    r = subprocess.run([cli, "--dump-records", str(path)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return parse_dump(r.stdout)


def test_cases_hold_what_they_name(programs):
    cli, _, files = programs
    e, x = S.edge_cases(), S.error_cases()
    for name, (_, kind, line) in x.items():
        assert dump(cli, files[name])[5:7] == (kind, line), name
    assert {k for _, k, _ in x.values()} == {S.HEADER_AFTER_RECORD, S.TOO_FEW_FIELDS, S.EMPTY_SEQ, S.BAD_LENGTHS}
    for name, (text, kind, line) in x.items():
        got = S.ref_walk(text, True, True)
        assert got[5:7] == (kind, line) and got[3] == line and got[4] == got[7], name
        assert got[0] == S.ref_walk(text[:got[7]], True, True)[0], name
    short, rich = x["a short line borrows no tab"][0].split(b"\n")[5:7]
    assert short.count(b"\t") == 9 and rich.count(b"\t") > 20
    for name, text in e.items():
        got = S.ref_walk(text, True, True)
        assert got[5] == S.OK and got[4] == len(text) and got[3] == len(S.lines_of(text, True)), name
    assert S.ref_walk(e["header only"], True, True)[:3] == ([], 4, len(S.HEADER))
    assert [r[4] for r in S.ref_walk(e["seq and qual are stars"], True, True)[0]] == [1, 0, 1]
    # not at the end, an unfinished line is the carry; behind the header, a '@' line is an error
    text = e["no final newline"]
    head = S.ref_walk(text, False, True)
    assert head[5] == S.OK and head[4] == text.rfind(b"\n") + 1 and head[0] == S.ref_walk(text, True, True)[0][:-1]
    assert S.ref_walk(e["header and records"], True, False)[5:7] == (S.HEADER_AFTER_RECORD, 0)
    # the same table from a text cut anywhere: what is not consumed is carried, the header state moves on
    text = e["generated"]
    whole = S.ref_walk(text, True, True)
    for cut in range(0, len(text), 97):
        a = S.ref_walk(text[:cut], False, True)
        b = S.ref_walk(text[a[4]:], True, a[1] == a[3])
        assert a[5] == b[5] == S.OK and a[0] + [(r[0] + a[4],) + r[1:] for r in b[0]] == whole[0]
        assert a[1] + b[1] == whole[1] and a[3] + b[3] == whole[3]


def test_bam_to_sam_conversion(programs, tmp_path):
    from tests.test_bam_subset import build_bam
    reads = [("kat", "TTAGGG" * 3), ("noseq", ""), ("odd", "ACGTN")]
    header, records, _ = build_bam(reads, 60000)
    text = S.bam_to_sam(header + b"".join(records))
    lines = text.split(b"\n")
    assert lines[:2] == [b"@HD\tVN:1.6\tSO:unsorted", b"@SQ\tSN:chr1\tLN:1000"]
    assert lines[2] == b"kat\t4\t*\t0\t0\t*\t*\t0\t0\t" + b"TTAGGG" * 3 + b"\t*"
    assert lines[3].split(b"\t")[9:] == [b"*", b"*"] and lines[4].split(b"\t")[9] == b"ACGTN"
    recs = S.ref_walk(text, True, True)
    assert recs[5] == S.OK and [r[4] for r in recs[0]] == [0, 1, 0]
    (tmp_path / "converted.sam").write_bytes(text)
    assert dump(programs[0], tmp_path / "converted.sam") == recs


def test_header_declares_and_library_exports_the_device_route():
    """Fails without the feature: include/teloscan.h states the rule and declares the entry points, libteloscan.so exports
    them, and the record's mirror has the C compiler's layout."""
    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", bare))
    assert set(NEW_ENTRY_POINTS) <= declared
    for code, value in (("TS_SAM_OK", S.OK), ("TS_SAM_HEADER_AFTER_RECORD", S.HEADER_AFTER_RECORD), ("TS_SAM_TOO_FEW_FIELDS", S.TOO_FEW_FIELDS),
                        ("TS_SAM_EMPTY_SEQ", S.EMPTY_SEQ), ("TS_SAM_BAD_LENGTHS", S.BAD_LENGTHS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (code, value), bare), code
    for msg in S.MESSAGES.values():
        assert msg in hdr, msg
    lib = C.CDLL(K.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert lib.ts_abi_version() == 4
    assert (K.SAM_OK, K.SAM_HEADER_AFTER_RECORD, K.SAM_TOO_FEW_FIELDS, K.SAM_EMPTY_SEQ, K.SAM_BAD_LENGTHS) == (0, 1, 2, 3, 4)


def test_record_mirror_matches_the_c_struct(tmp_path):
    from teloscope_amd import _capi as K
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "teloscan.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(ts_sam_record), offsetof(ts_sam_record, off), offsetof(ts_sam_record, seq_at), '
                   'offsetof(ts_sam_record, seq_len), offsetof(ts_sam_record, size), offsetof(ts_sam_record, flags));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = K.SamRecord
    assert got == [C.sizeof(R), R.off.offset, R.seq_at.offset, R.seq_len.offset, R.size.offset, R.flags.offset] and got[0] == 24


def test_cli_refuses_without_a_device(programs):
    from teloscope_amd import _capi as K
    cli, _, files = programs
    r = subprocess.run([cli, "-x", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--sam-subset" in r.stderr
    if K.lib().ts_device_count() > 0:
        return                                                   # (with a device: tests/test_gpu_sam_device.py)
    for route in ("--device", "--host"):
        r = subprocess.run([cli, "--sam-subset", route, str(files["header and records"])], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr and r.stdout == ""
