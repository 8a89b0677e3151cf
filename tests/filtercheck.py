"""What tests/test_filter_check_reference_cpu.py, tests/test_gpu_filter_check.py and tests/test_gpu_filter_device.py share:
plain-Python statements of the two device checks behind the assembly record filters (ts_gfa_chunk_check,
ts_fasta_chunk_strict) and of the filtered loaders' verdicts they serve, seeded generators of lines and records, thin ctypes
wrappers over the two entry points, and the build of tests/cpp/assembly_device_cli.cpp.  No test functions live here.

The references restate the host route (validateFilteredGfa in include/teloscope_mi355x_gfa.hpp, FastaGroupReader::checkStrict
in include/teloscope_mi355x_io.hpp), not the kernels: they go through the text line by line and through a body byte by byte."""
import ctypes as C
import os
import random
import subprocess

from tests import fastachunk as F
from tests import gfachunk as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DECIDES = 255
GFA2 = "; use GFA1 P paths or a pathless GFA1 graph."
NOT_FASTA = "Assembly record filters require FASTA input or a recognized GFA file."


# ------------------------------------------------------------------------------------------------------------ GFA
def gfa_rule(line):
    """validateFilteredGfa's verdict on one line whose '\\r' bytes are gone: 0, or the first rule it breaks (1..7)."""
    line = bytes(line)
    if not line or line[:1] == b"#":
        return 0
    if line[:2] == b"H\t" and b"\tVN:Z:2" in line:
        return 1
    if len(line) < 2 or line[1:2] != b"\t":
        return 2
    t = line[:1]
    if t in (b"O", b"U", b"E", b"G", b"F"):
        return 3
    if t == b"W":
        return 4
    if t == b"C":
        return 5
    if t == b"S":
        t2 = line.find(b"\t", 2)
        t3 = line.find(b"\t", t2 + 1) if t2 >= 0 else -1
        if t3 >= 0 and t3 > t2 + 1 and all(48 <= c <= 57 for c in line[t2 + 1:t3]):
            return 6
    if t not in (b"H", b"S", b"L", b"J", b"P"):
        return 7
    return 0


def gfa_message(code, type_byte, line_no):
    """The SequenceFilterError text of a broken rule."""
    at, t = " at line %d" % line_no, chr(type_byte)
    return {1: "Assembly record filters do not support GFA2" + at + GFA2,
            2: "Assembly record filters found a malformed or unsupported GFA record" + at + ".",
            3: "Assembly record filters do not support GFA2 record type '" + t + "'" + at + GFA2,
            4: "Assembly record filters do not support GFA1 W walks" + at + GFA2,
            5: "Assembly record filters do not support GFA1 C containment records" + at + ".",
            6: "Assembly record filters do not support GFA2 segment records" + at + GFA2,
            7: "Assembly record filters do not support GFA record type '" + t + "'" + at + "."}[code]


def gfa_lines(text, at_end):
    """(begin, content end) of every whole line: the content is without the '\\n' and ONE '\\r' in front of it (or, at the
    input's end, in front of nothing); an unfinished last line counts only with at_end."""
    text = bytes(text)
    out, p, n = [], 0, len(text)
    while p < n:
        nl = text.find(b"\n", p)
        if nl < 0 and not at_end:
            break
        e, q = (n, n) if nl < 0 else (nl, nl + 1)
        if e > p and text[e - 1] == 13:
            e -= 1
        out.append((p, e))
        p = q
    return out


def ref_gfa_check(text, at_end):
    """ts_gfa_chunk_check: -> (n_lines, [(line ordinal, off, len, code, type)]).  A line with a '\\r' inside its content is the
    host's (255) whatever else it holds; otherwise the rule of the line as it lies."""
    text = bytes(text)
    lines = gfa_lines(text, at_end)
    flagged = []
    for i, (b, e) in enumerate(lines):
        c = text[b:e]
        code = HOST_DECIDES if b"\r" in c else gfa_rule(c)
        if code:
            flagged.append((i, b, e - b, code, text[b] if b < len(text) else 0))
    return len(lines), flagged


def ref_gfa_offence(text):
    """The filtered loader's verdict on a whole text: None, or the message of its first offending line (the host judges the
    lines the device hands back)."""
    text = bytes(text)
    for i, (b, e) in enumerate(gfa_lines(text, True)):
        line = text[b:e].replace(b"\r", b"")
        code = gfa_rule(line)
        if code:
            return gfa_message(code, line[0], i + 1)
    return None


def gfa_probe_lines(seed=3):
    """A few hundred single lines (no line end): every type letter alone, with a tab and with a field; S lines with a digit,
    non-digit or empty third field; H lines with and without VN:Z:2; '\\r' inside a line."""
    gen = random.Random(seed)
    out = [b"", b"#", b"# a comment", b"#\tS\tx\t12\tAC", b"\t", b"\t\t", b"S", b"S\t", b"H", b"H\t", b"SX\ta\tAC", b" S\ta\tAC"]
    for t in range(33, 127):
        c = bytes([t])
        out += [c, c + b"\tx", c + b"\tname\tACGT\t*", c + b"x\ty"]
    for third in (b"4", b"0123456789", b"", b"4a", b"a4", b"ACGT", b"*", b"-4", b"4 ", b"12\r"):
        out += [b"S\tn\t" + third + b"\tACGT", b"S\tn\t" + third, b"S\tn\t" + third + b"\t", b"S\t\t" + third + b"\tAC\tLN:i:2"]
    for tag in (b"VN:Z:2.0", b"VN:Z:2", b"VN:Z:1.0", b"VN:Z:12", b"vn:Z:2.0", b"VN:Z:", b"xVN:Z:2", b"VN:Z:\t2"):
        out += [b"H\t" + tag, b"H\tfoo:Z:bar\t" + tag, b"H\t" + tag + b"\tzz:i:1", b"H" + tag, b"Hx\t" + tag, b"S\tn\tAC\t" + tag,
                b"L\ta\t+\tb\t-\t0M\t" + tag]
    for line in (b"S\ta\tAC\rGT", b"S\r\ta\tACGT", b"\rS\ta\tACGT", b"O\r\tx", b"\rO\tx", b"#\rx", b"\r#", b"\r", b"\r\r", b"H\tVN:Z:\r2.0",
                 b"H\tVN\r:Z:2", b"S\tn\t1\r2\tAC", b"S\tn\t\r\tAC", b"X\r", b"W\tx\r\ty", b"S\ta\tAC\r\r"):
        out.append(line)
    for _ in range(40):
        out.append(bytes(gen.choice(b"SHLPJWCOX#\t\r012 a") for _ in range(gen.randrange(1, 9))))
    return out


def gfa_text(lines, eol=b"\n", last_eol=True):
    return eol.join(lines) + (eol if last_eol and lines else b"")


# ------------------------------------------------------------------------------------------------------------ FASTA
def ref_has_sequence(text, recs):
    """ts_fasta_chunk_strict: per record (tuples of fastachunk.ref_walk), 1 when its body text holds a byte other than '\\n' and
    '\\r'."""
    text = bytes(text)
    return [1 if text[r[0] + r[2]:r[0] + r[1]].strip(b"\r\n") else 0 for r in recs]


def primary_id(name):
    for i, c in enumerate(name):
        if c in b" \t\r\n\f\v":
            return name[:i]
    return name


def ref_fasta_offence(text):
    """The filtered FASTA loader's verdict (FastaGroupReader::checkStrict) on a whole text: None, or its message."""
    text = bytes(text)
    if text[:3] == b"\xef\xbb\xbf":
        text = text[3:]
    recs, _, names = F.ref_walk(text, True)
    if (recs[0][0] != 0) if recs else len(text) > 0:
        return NOT_FASTA
    has = ref_has_sequence(text, recs)
    ids = [primary_id(names[r[4]:r[4] + r[5]]).decode("latin-1") for r in recs]
    seen = set()
    for i, name in enumerate(ids):
        if i and not has[i - 1]:
            return "FASTA record '%s' has no sequence." % ids[i - 1]
        if not name:
            return "FASTA input contains an empty primary sequence ID."
        if name in seen:
            return "Input contains duplicate primary sequence ID: '%s'." % name
        seen.add(name)
    if not recs:
        return "Assembly input is empty."
    if not has[-1]:
        return "FASTA record '%s' has no sequence." % ids[-1]
    return None


BODIES = [b"", b"\n", b"\n\n", b"\r\n", b"\r\r\n", b"\r", b"\r\r", b"\n\r\n\r", b"A\n", b"\nA\n", b"\r\nA", b" \n", b"\tx\r\n", b"N\n",
          b"\r\r\rA\r\n", b"\n" * 70 + b"c\n", b"ACGT\nACGT\n"]


def fasta_probe_texts(seed=4):
    """Complete FASTA texts: every body of BODIES as a first, a middle and a last record; bytes in front of the first header; no
    record; duplicate and empty IDs; a byte order mark; and some generated ones."""
    gen = random.Random(seed)
    out = [b"", b"\xef\xbb\xbf", b"\n", b"ACGT\n", b"\xef\xbb\xbf\n>a\nAC\n", b"\xef\xbb\xbf>a\nAC\n", b" >a\nAC\n", b">a\nAC\n>a\nGT\n",
           b">a x\nAC\n>b\nGT\n>a\ty\nAA\n", b">\nAC\n", b"> a\nAC\n", b">a\nAC\n>\x0bb\nGT\n", b">a\x0cb\nAC\n>a\nGT\n", b">a\r\nAC\r\n>a\r\nGT\r\n",
           b">a\n>a\nAC\n", b">\n>\n", b">a", b">a\r", b">a\nAC", b">a\nAC\r", b">a\n\r"]
    for body in BODIES:
        out += [b">a\n" + body + b">b\nAC\n", b">a\nAC\n>b\n" + body + b">c\nGT\n", b">a\nAC\n>b\n" + body]
    for _ in range(30):
        recs = []
        for i in range(gen.randrange(1, 6)):
            name = gen.choice([b"r%d" % i, b"r%d words" % i, b"r0", b"", b"r%d\tx" % i])
            recs.append(b">" + name + gen.choice([b"\n", b"\r\n"]) + gen.choice(BODIES))
        out.append(gen.choice([b"", b"", b"", b"\n", b"x\n"]) + b"".join(recs))
    return out


# -------------------------------------------------------------------------------------------- the library through ctypes
class Chunk(G.Chunk):
    """A ts_chunk fed with plain text, the GFA walk over it, and the two checks."""

    def gfa_check(self, at_end, cap=1 << 12):
        """-> (rc, n_lines, flagged as ref_gfa_check gives them, *n_flagged); what lies behind the entries taken must be as it
        was."""
        K = self.K
        arr = (K.GfaFlagged * (cap + 1))()
        C.memset(arr, 0xEE, C.sizeof(arr))
        nf, nl = C.c_uint64(7), C.c_uint64(7)
        rc = self.L.ts_gfa_chunk_check(self.ptr, 1 if at_end else 0, arr, cap, C.byref(nf), C.byref(nl))
        if rc != K.TS_OK:
            rest = bytes(arr)
            assert rest == b"\xee" * len(rest), "a refused check wrote entries"
            return rc, nl.value, [], nf.value
        assert nf.value <= cap
        got = [(e.line, e.off, e.len, e.code, e.type) for e in arr[:nf.value]]
        rest = bytes(arr)[nf.value * C.sizeof(K.GfaFlagged):]
        assert rest == b"\xee" * len(rest), "the check wrote behind the entries it reported"
        return rc, nl.value, got, nf.value

    def walk_and_check(self, text, at_end):
        """The chunk, which holds `text`, walked (the check works on a walked chunk) and checked -> (n_lines, flagged, next)."""
        rc, segs, lines, gathered, nxt, foreign, counts = self.gfa_walk(at_end, seg_cap=text.count(b"\n") + 2, line_cap=text.count(b"\n") + 2,
                                                                        text_cap=len(text) + 16)
        assert rc == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        rc, n_lines, flagged, nf = self.gfa_check(at_end, cap=text.count(b"\n") + 2)
        assert rc == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        return n_lines, flagged, nxt

    def fasta_strict(self, records, stream=None):
        """-> has_sequence of the records (tuples of fasta_walk), as a list; the byte behind the last one must be as it was."""
        n = len(records)
        buf = C.create_string_buffer(b"\xee" * (n + 1), n + 1)
        rc = self.L.ts_fasta_chunk_strict(self.ptr, F.table_of(records), n, buf, stream)
        assert rc == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        assert buf.raw[n:] == b"\xee", "the strict check wrote behind its records"
        return list(buf.raw[:n])


def build_driver(out):
    """tests/cpp/assembly_device_cli.cpp -> the binary at `out`."""
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "assembly_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)
