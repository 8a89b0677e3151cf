"""What tests/test_fasta_chunk_reference_cpu.py and tests/test_gpu_fasta_chunk.py share: a plain-Python sequential restatement
of the FASTA stages (ref_walk, ref_join, ref_runs), seeded generators of FASTA text with their edge cases, and thin ctypes
wrappers over the ts_fasta_chunk_* entry points.  No test functions live here.

The references restate the host route (readFasta / FastaGroupReader / splitPath in include/teloscope_mi355x_io.hpp), not the
kernels: they go through the text line by line and through a record's bases byte by byte.  The device does the same with a
line index, prefix sums over lines and a stream compaction."""
import ctypes as C
import random
import re

from tests import bamchunk as B
from tests import fastqchunk as FQ

GAP_LETTERS = b"NnXx"


# ------------------------------------------------------------------------------------------------------------ references
def _lines(text, at_end):
    """(begin, end without the newline, has a newline) of every line; an unfinished last line counts only at the input's end."""
    out, p, n = [], 0, len(text)
    while p < n:
        nl = text.find(b"\n", p)
        if nl < 0:
            if at_end:
                out.append((p, n, False))
            break
        out.append((p, nl, True))
        p = nl + 1
    return out


def _logical_end(text, b, e, at_end, has_nl):
    """The line's end without a carriage return in front of its newline (or, at the input's very end, in front of nothing)."""
    if e > b and text[e - 1] == 13 and (has_nl or (at_end and e == len(text))):
        return e - 1
    return e


def ref_walk(text, at_end):
    """-> (records, next, names): a record is (off, text_len, body_at, n_bases, name_at, name_len) as ts_fasta_record holds it;
    names is the complete records' header lines (without '>' and line end) one behind the other."""
    text = bytes(text)
    n = len(text)
    lines = _lines(text, at_end)
    heads = [i for i, (b, e, _) in enumerate(lines) if e > b and text[b] == 62]
    recs, names = [], bytearray()
    if not heads:
        last_line = lines[-1][1] + 1 if lines and lines[-1][2] else (lines[-1][0] if lines else 0)
        return [], (n if at_end else last_line), b""
    for k, i in enumerate(heads):
        b, e, has_nl = lines[i]
        stop = lines[heads[k + 1]][0] if k + 1 < len(heads) else n
        body = min(e + 1, n) if has_nl else n
        bases = 0
        for lb, le, nl in lines[i + 1:(heads[k + 1] if k + 1 < len(heads) else len(lines))]:
            bases += _logical_end(text, lb, le, at_end, nl) - lb
        name = text[b + 1:_logical_end(text, b, e, at_end, has_nl)]
        recs.append((b, stop - b, body - b, bases, len(names), len(name)))
        names += name
    if at_end:
        return recs, n, bytes(names)
    open_rec = recs.pop()                               # the next chunk may continue it
    return recs, open_rec[0], bytes(names[:open_rec[4]])


def ref_bases(text, rec, at_end=True):
    """A record's bases: its body text without '\\n', a '\\r' right before one, and a '\\r' that is the input's last byte."""
    text = bytes(text)
    off, text_len, body_at = rec[:3]
    body = text[off + body_at:off + text_len]
    ends_input = off + text_len == len(text) and at_end
    parts = body.split(b"\n")
    out = []
    for k, line in enumerate(parts):
        if line.endswith(b"\r") and (k + 1 < len(parts) or ends_input):
            line = line[:-1]
        out.append(line)
    return b"".join(out)


def ref_join(text, recs, at_end=True):
    """-> (the joined buffer: record i at offsets[i], a multiple of 16, zeros between; offsets)"""
    img, offsets = bytearray(), []
    for r in recs:
        offsets.append(len(img))
        bases = ref_bases(text, r, at_end)
        assert len(bases) == r[3], (r, len(bases))
        img += bases + bytes(-len(bases) % 16)
    return bytes(img), offsets


def ref_runs_of(bases):
    """[(is_gap, start, len)] of one record's bases, byte by byte."""
    runs = []
    for i, c in enumerate(bases):
        g = 1 if c in GAP_LETTERS else 0
        if runs and runs[-1][0] == g:
            runs[-1][2] += 1
        else:
            runs.append([g, i, 1])
    return [tuple(r) for r in runs]


def ref_runs(text, recs, at_end=True):
    """-> [(record, is_gap, start, len)] as ts_fasta_run holds them"""
    return [(i,) + run for i, r in enumerate(recs) for run in ref_runs_of(ref_bases(text, r, at_end))]


def name_word(line):
    """What the host keeps of a header line: up to the first space or tab."""
    return re.split(b"[ \t]", line, 1)[0]


# ------------------------------------------------------------------------------------------------------------ generators
def random_bases(gen, n, gaps=True):
    out = bytearray(gen.choice(b"ACGTacgt") for _ in range(n))
    if gaps and n > 40:
        for _ in range(gen.randrange(0, 4)):
            a = gen.randrange(0, n - 20)
            ln = gen.randrange(1, 20)
            out[a:a + ln] = bytes(gen.choice(GAP_LETTERS) for _ in range(ln)) if gen.random() < 0.3 else b"N" * ln
    return bytes(out)


def fold(bases, width, eol=b"\n", last_eol=True):
    lines = [bases[a:a + width] for a in range(0, len(bases), width)]
    text = eol.join(lines)
    return text + (eol if last_eol and lines else b"")


def record_text(name, bases, width=60, eol=b"\n", last_eol=True):
    return b">" + name + eol + fold(bases, width, eol, last_eol)


def assembly_text(seed, n_records, lo=0, hi=3000, eol=b"\n", widths=(60, 80, 61, 17)):
    gen = random.Random(seed)
    out = []
    for i in range(n_records):
        n = 0 if i % 11 == 7 else gen.randrange(lo, hi)
        out.append(record_text(b"seq%d_%d description\twith tab" % (seed, i), random_bases(gen, n), widths[i % len(widths)], eol))
        if i % 9 == 4:
            out.append(eol)                             # a blank line behind a record
    return b"".join(out)


def edge_cases():
    """name -> complete text."""
    gen = random.Random(5)
    a, b = random_bases(gen, 500), random_bases(gen, 333)
    cases = {}
    for w in (1, 15, 16, 17, 60, 61, 80):
        cases["width %d" % w] = record_text(b"w%d" % w, a, w) + record_text(b"second", b, w)
    cases["one line of 20000 bases"] = record_text(b"long", random_bases(gen, 20000), 20000) + record_text(b"b", b)
    cases["crlf"] = record_text(b"w", a, 60, b"\r\n") + record_text(b"x y", b, 61, b"\r\n")
    cases["blank and cr-only lines in a body"] = b">r\nACGT\n\n\r\nNNAC\n\n>s\n\r\n\n\nAC\r\nGT\n"
    cases["no final newline"] = record_text(b"a", a) + record_text(b"b", b, 60, b"\n", False)
    cases["no final newline, final cr"] = record_text(b"a", a) + record_text(b"b", b, 60, b"\r\n", False) + b"\r"
    cases["no final newline, crlf"] = record_text(b"a", a, 60, b"\r\n") + record_text(b"b", b, 60, b"\r\n", False)
    cases["header without newline at the end"] = record_text(b"a", a) + b">lonely"
    cases["header with cr at the end"] = record_text(b"a", a) + b">lonely\r"
    cases["gt in mid-line"] = b">r >x\nAC>GT\nA>\n>s\n>t\nACGT>\n"
    cases["text in front of the first header"] = b"stray text\nACGT\n\n" + record_text(b"a", a) + record_text(b"b", b)
    cases["names with spaces, tabs and cr"] = b">n1 some words\r\nACGT\r\n>n2\twith tab\nACGT\n>\nAC\n> lead\nGT\n>n5\r\r\nAA\n"
    cases["record with no body"] = b">a\n>b\nACGT\n>c\n"
    cases["body of blank lines only"] = b">a\n\n\n\r\n>b\nACGT\n"
    cases["two records back to back"] = b">a\nAC\n>b\nGT\n"
    cases["stray cr inside a line"] = b">a\nAC\rGT\r\rA\nNN\r\n"
    cases["space is a base"] = b">a\nAC GT\n  \nN N\n"
    cases["one gap"] = b">g\nNNNNNNNNNNNNNNNNNNNNNNNNNNNN\nNNNN\n>h\nACGT\n"
    cases["gaps at both ends of neighbours"] = b">a\nNNACGTNN\n>b\nNNACGTNN\n>c\nnnACxx\n"
    cases["anan"] = record_text(b"alt", b"AN" * 2300 + b"A", 80)
    cases["all gap letters"] = b">m\nACNnXxGTnNxXAC\nxnXN\n"
    cases["only a header"] = b">only\n"
    cases["no header at all"] = b"ACGT\nACGT\n"
    # (seeds with which pieces of 37 bytes end in a header, in a body line, right behind a newline and right before a '>':
    # tests/test_gpu_fasta_chunk.py asserts that they do)
    cases["generated"] = assembly_text(3, 40)
    cases["generated crlf"] = assembly_text(6, 30, eol=b"\r\n")
    return cases


# -------------------------------------------------------------------------------------------- the library through ctypes
def table_of(records):
    from teloscope_amd import _capi as K
    arr = (K.FastaRecord * max(1, len(records)))()
    for i, (off, text_len, body_at, n_bases, name_at, name_len) in enumerate(records):
        r = arr[i]
        r.off, r.text_len, r.body_at, r.n_bases, r.name_at, r.name_len = off, text_len, body_at, n_bases, name_at, name_len
    return arr


class Chunk(FQ.Chunk):
    """A ts_chunk fed with plain text or BGZF members, and the FASTA stages over it."""

    def fasta_walk(self, at_end, cap=1 << 12, names_cap=1 << 16):
        """-> (rc, records as tuples, next, names bytes, *n, *names_bytes); what lies behind the records and names taken must
        be as it was."""
        K = self.K
        arr = (K.FastaRecord * (cap + 1))()
        C.memset(arr, 0xEE, C.sizeof(arr))
        names = C.create_string_buffer(b"\xee" * (names_cap + 8), names_cap + 8)
        n, nxt, nb = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        rc = self.L.ts_fasta_chunk_walk(self.ptr, 1 if at_end else 0, arr, cap, C.byref(n), C.byref(nxt), names, names_cap, C.byref(nb))
        if rc != K.TS_OK:
            return rc, [], nxt.value, b"", n.value, nb.value
        assert n.value <= cap and nb.value <= names_cap
        recs = []
        for i in range(n.value):
            assert arr[i].reserved == 0
            recs.append((arr[i].off, arr[i].text_len, arr[i].body_at, arr[i].n_bases, arr[i].name_at, arr[i].name_len))
        rest = bytes(arr)[n.value * C.sizeof(K.FastaRecord):]
        assert rest == b"\xee" * len(rest), "the walk wrote behind the records it reported"
        assert names.raw[nb.value:] == b"\xee" * (names_cap + 8 - nb.value), "the walk wrote behind the names it reported"
        return rc, recs, nxt.value, names.raw[:nb.value], n.value, nb.value

    def fasta_join(self, records, at_end, stream=None):
        """-> (rc, device pointer, offsets, total bytes, runs)"""
        n = len(records)
        d, offs = C.c_void_p(0), (C.c_uint64 * max(1, n))()
        total, runs = C.c_uint64(0xdead), C.c_uint64(0xdead)
        rc = self.L.ts_fasta_chunk_join(self.ptr, table_of(records), n, 1 if at_end else 0, C.byref(d), offs, C.byref(total),
                                        C.byref(runs), stream)
        return rc, d.value, [int(offs[i]) for i in range(n)], total.value, runs.value

    def fasta_runs(self, cap):
        """-> (rc, runs as tuples, *n_runs)"""
        K = self.K
        arr = (K.FastaRun * (cap + 1))()
        C.memset(arr, 0xEE, C.sizeof(arr))
        n = C.c_uint64(7)
        rc = self.L.ts_fasta_chunk_runs(self.ptr, arr, cap, C.byref(n))
        if rc != K.TS_OK:
            return rc, [], n.value
        rest = bytes(arr)[n.value * C.sizeof(K.FastaRun):]
        assert rest == b"\xee" * len(rest), "the runs were written behind their count"
        return rc, [(arr[i].record, arr[i].is_gap, arr[i].start, arr[i].len) for i in range(n.value)], n.value

    def fasta_bases(self, off, n):
        buf = C.create_string_buffer(max(n, 1))
        assert self.L.ts_fasta_chunk_bases(self.ptr, off, n, buf) == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        return buf.raw[:n]


__all__ = ["B", "FQ"]
