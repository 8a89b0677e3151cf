"""The plain-Python statements of the two device checks behind the assembly record filters (tests/filtercheck.py) pinned by the
host route, without a device: tests/cpp/assembly_device_cli.cpp --host --selection-only must refuse and accept, with the same
words, as the Python rules say — on the GFA rejections and FASTA loader cases of tests/test_record_filters.py (copied here as
data) and on a few hundred generated lines and records.  Also: the two entry points are declared, exported and bound, and the
driver builds."""
import ctypes as C
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import filtercheck as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/test_record_filters.py: GFA_REJECTIONS (the entries that reach the line rules) and test_fasta_loader_errors
GFA_REJECTIONS = [
    (b"# c\nH\tVN:Z:2.0\nS\ta\t4\tACGT\n",
     "Assembly record filters do not support GFA2 at line 2; use GFA1 P paths or a pathless GFA1 graph."),
    (b"H\tVN:Z:1.0\nS\ta\tACGT\nO\to1\ta+\n",
     "Assembly record filters do not support GFA2 record type 'O' at line 3; use GFA1 P paths or a pathless GFA1 graph."),
    (b"H\tVN:Z:1.1\nS\ta\tACGT\nW\tsm\t0\tc\t0\t4\t>a\n",
     "Assembly record filters do not support GFA1 W walks at line 3; use GFA1 P paths or a pathless GFA1 graph."),
    (b"S\ta\tACGT\nS\tb\tAC\nC\ta\t+\tb\t+\t0\t2M\n",
     "Assembly record filters do not support GFA1 C containment records at line 3."),
    (b"S\ta\t4\tACGT\n",
     "Assembly record filters do not support GFA2 segment records at line 1; use GFA1 P paths or a pathless GFA1 graph."),
    (b"S\ta\tACGT\nX\tfoo\n", "Assembly record filters do not support GFA record type 'X' at line 2."),
    (b"S\ta\tACGT\nSx\tb\n", "Assembly record filters found a malformed or unsupported GFA record at line 2."),
]
FASTA_LOADER_CASES = [
    (b">a x\nACGT\n>b\nACGT\n>a\ty\nACGT\n", "Input contains duplicate primary sequence ID: 'a'."),
    (b">a\n>b\nACGT\n", "FASTA record 'a' has no sequence."),
    (b">a\nACGT\n>b\n\n", "FASTA record 'b' has no sequence."),
    (b">a\nACGT\n> b\nACGT\n", "FASTA input contains an empty primary sequence ID."),
    (b"@r1\nACGT\n+\nIIII\n", FC.NOT_FASTA),
    (b"\n>a\nACGT\n", FC.NOT_FASTA),
    (b"", "Assembly input is empty."),
]
STRICT_WORDS = ("FASTA record '", "FASTA input contains an empty", "Input contains duplicate primary sequence ID:", "Assembly input is empty.",
                FC.NOT_FASTA)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return FC.build_driver(tmp_path_factory.mktemp("cpp") / "assembly_device_cli")


def verdicts(driver, tmp_path, suffix, texts, *filters):
    """The host route's last stderr line for every text (each its own file), eight runs side by side."""
    import subprocess

    def one(k):
        p = tmp_path / ("t%04d%s" % (k, suffix))
        p.write_bytes(texts[k])
        r = subprocess.run([driver, "--host", str(p), "--selection-only"] + list(filters), stdin=subprocess.DEVNULL, capture_output=True, timeout=60)
        lines = r.stderr.decode("latin-1").splitlines()
        return r.returncode, lines[-1] if lines else ""
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(one, range(len(texts))))


def test_entry_points_declared_exported_and_bound():
    from teloscope_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "teloscan.h")).read(), flags=re.S)
    lib = C.CDLL(_capi.LIB_PATH)
    for name in ("ts_fasta_chunk_strict", "ts_gfa_chunk_check"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _capi.SYMBOLS
    assert re.search(r"#define\s+TS_GFA_CHECK_HOST_DECIDES\s+255\b", hdr) and _capi.GFA_CHECK_HOST_DECIDES == FC.HOST_DECIDES == 255
    assert C.sizeof(_capi.GfaFlagged) == 24


def test_reference_says_what_the_copied_cases_say():
    for text, message in GFA_REJECTIONS:
        assert FC.ref_gfa_offence(text) == message
    for text, message in FASTA_LOADER_CASES:
        assert FC.ref_fasta_offence(text) == message


def test_check_reference_agrees_with_the_loader_reference():
    """ref_gfa_check (what the device answers) resolved as the route resolves it — a 255 line judged by the loader's rule on the
    line without its '\\r' — names the loader's first offence, on every probe line in every framing."""
    lines = FC.gfa_probe_lines()
    texts = [FC.gfa_text(lines), FC.gfa_text(lines, b"\r\n"), FC.gfa_text(lines, b"\n", False), FC.gfa_text(lines[::-1], b"\r\n", False)]
    texts += [FC.gfa_text([b"S\tkeepme\tACGT", l]) for l in lines]
    assert sum(1 for l in lines if FC.gfa_rule(l.replace(b"\r", b""))) > 100 and sum(1 for l in lines if b"\r" in l) > 10
    for text in texts:
        n_lines, flagged = FC.ref_gfa_check(text, True)
        assert n_lines == len(text.split(b"\n")) - (1 if text.endswith(b"\n") or not text else 0)
        first = None
        for i, off, ln, code, typ in flagged:
            line = text[off:off + ln].replace(b"\r", b"")
            code = FC.gfa_rule(line) if code == FC.HOST_DECIDES else code
            if code:
                first = FC.gfa_message(code, line[0], i + 1)
                break
        assert first == FC.ref_gfa_offence(text)


def test_gfa_rules_pinned_by_the_host_route(driver, tmp_path):
    lines = FC.gfa_probe_lines()
    texts = [t for t, _ in GFA_REJECTIONS]
    texts += [FC.gfa_text([b"S\tkeepme\tACGT", l]) for l in lines]
    texts += [FC.gfa_text([b"S\tkeepme\tACGT", l], b"\r\n") for l in lines[::3]]
    texts += [FC.gfa_text([b"S\tkeepme\tACGT", b"", b"# c", l], b"\n", False) for l in lines[1::3]]
    got = verdicts(driver, tmp_path, ".gfa", texts, "--include-prefix", "keepme")
    refused = 0
    for text, (rc, last) in zip(texts, got):
        want = FC.ref_gfa_offence(text)
        if want is None:
            assert "Assembly record filters" not in last, (text, last)
        else:
            assert rc == 1 and last == "Error: " + want, (text, last, want)
            refused += 1
    assert refused > 150 and len(texts) - refused > 100
    for (_, message), (rc, last) in zip(GFA_REJECTIONS, got):
        assert last == "Error: " + message


def test_fasta_rules_pinned_by_the_host_route(driver, tmp_path):
    texts = [t for t, _ in FASTA_LOADER_CASES] + FC.fasta_probe_texts()
    got = verdicts(driver, tmp_path, ".fa", texts, "--include-prefix", "a,r")
    refused = 0
    for text, (rc, last) in zip(texts, got):
        want = FC.ref_fasta_offence(text)
        if want is None:
            assert not any(w in last for w in STRICT_WORDS), (text, last)
        else:
            assert rc == 1 and last == "Error: " + want, (text, last, want)
            refused += 1
    assert refused > 40 and len(texts) - refused > 20
    for body in FC.BODIES:                                       # has_sequence is not n_bases > 0
        text = b">a\n" + body
        has = FC.ref_has_sequence(text, [(0, len(text), 3, 0, 0, 1)])
        assert has == [1 if body.replace(b"\r", b"").replace(b"\n", b"") else 0]
