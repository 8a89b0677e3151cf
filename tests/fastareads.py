"""What tests/test_fasta_reads_reference_cpu.py, tests/test_gpu_fasta_reads_chunk.py and tests/test_gpu_fasta_reads_device.py
share: a plain-Python restatement of the FASTA read subset's rule (include/teloscan.h above ts_fasta_chunk_stage) on top of
tests/fastachunk.py's ref_walk / ref_bases — the stage's input image, the gather, the block report's names and the whole route —
a writer of reads as FASTA text, the edge cases of the rule, and thin ctypes wrappers over the three entry points.  No test
functions live here.

The references go through a record's text byte by byte and share nothing with the kernels: the device counts kept bytes per
slice of body text, places the slices by prefix sums and copies spans."""
import ctypes as C
import re

from tests import fastachunk as F

EMPTY = "FASTA input is empty"
NO_HEADER = "FASTA input must start with '>'"


# ------------------------------------------------------------------------------------------------------------ references
def ref_stage(offsets, input_bytes, text, recs, at_end=True):
    """The batch's input buffer after the stage: recs[i]'s bases at offsets[i], every other byte zero."""
    img = bytearray(input_bytes)
    for off, r in zip(offsets, recs):
        bases = F.ref_bases(text, r, at_end)
        assert len(bases) == r[3] > 0 and off + len(bases) <= input_bytes
        img[off:off + len(bases)] = bases
    return bytes(img)


def record_text(text, rec):
    """A record as it is written: its text, and a newline when it lacks one (only the input's last record can)."""
    t = bytes(text[rec[0]:rec[0] + rec[1]])
    return t if t.endswith(b"\n") else t + b"\n"


def ref_gather(text, recs, pass_bytes):
    """-> (the passing records as they are written, in input order; how many they are)"""
    kept = [record_text(text, r) for r, p in zip(recs, pass_bytes) if p]
    return b"".join(kept), len(kept)


def ref_name(text, rec):
    """The block report's name: the header line behind '>' (ts_fasta_record's name_len bytes) up to the first space or tab."""
    return re.split(b"[ \t]", bytes(text[rec[0] + 1:rec[0] + 1 + rec[5]]), 1)[0]


def ref_names(text, recs):
    return [ref_name(text, r) for r in recs]


def ref_subset(text, read_filter):
    """The whole route on a complete text: (stdout bytes, (total, kept, without sequence), message or None, [(name, bases)] of
    the records judged, in order: what tests/readblocks.py's ref_report makes the block report from)."""
    text = bytes(text)
    if not text:
        return b"", (0, 0, 0), EMPTY, []
    if text[:1] != b">":
        return b"", (0, 0, 0), NO_HEADER, []
    recs, nxt, _ = F.ref_walk(text, True)
    assert nxt == len(text) and recs and recs[0][0] == 0
    with_seq = [r for r in recs if r[3] > 0]
    reads = [F.ref_bases(text, r) for r in with_seq]
    passes = read_filter.filter(reads) if reads else []
    out, kept = ref_gather(text, with_seq, passes)
    return out, (len(recs), kept, len(recs) - len(with_seq)), None, list(zip(ref_names(text, with_seq), reads))


def figures(stats):
    total, kept, missing = stats
    return "FASTA subset: kept %d of %d records (%d without sequence)." % (kept, total, missing)


def kept_names(out):
    """The names of the records of a subset (no body line of these tests begins with '>')."""
    return [re.split(b"[ \t\r]", l[1:], 1)[0].decode() for l in out.split(b"\n") if l.startswith(b">")]


# ------------------------------------------------------------------------------------------------------------ writers
def reads_text(reads, width=None, eol=b"\n", names=None, last_eol=True):
    """The reads as records r0, r1, ... (or `names`), body lines of `width` bases (None: one line per read)."""
    out = []
    for i, r in enumerate(reads):
        name = b"r%d" % i if names is None else names[i]
        out.append(F.record_text(name, r, width or max(len(r), 1), eol))
    text = b"".join(out)
    return text if last_eol or not text.endswith(eol) else text[:-len(eol)]


def edge_cases():
    """name -> complete text that starts with '>': the rule's corners, for the framing, the stage and the gather."""
    t = b"TTAGGG" * 9
    cases = {
        "a body of no lines": b">a\n>b\n" + t + b"\n>c\n",
        "a body of blank lines only": b">a\n\n\r\n\n>b\n" + t + b"\n",
        "one line without newline at the end": b">a\n" + t + b"\n>b\n" + t,
        "a cr as the input's last byte": b">a\n" + t + b"\n>b\n" + t + b"\r",
        "a cr and no bases at the end": b">a\n" + t + b"\n>b\n\r",
        "a gt inside a body line": b">a >x\nTTAGGG>TTAGGG\n" + t + b">\n>b\n>c\n" + t + b"\n",
        "a header alone at the end": b">a\n" + t + b"\n>lonely",
        "a header with cr alone at the end": b">a\n" + t + b"\n>lonely\r",
        "only a header": b">only\n",
        "only a gt": b">",
        "blank lines between and behind records": b">a\n" + t + b"\n\n\n>b\n\n" + t + b"\n\n",
        "stray cr inside a line": b">a\nTTAGGG\rTTAGGG\r\r\n" + t + b"\n",
        "a space is a base": b">a\nTTAGGG TTAGGG\n  \n" + t + b"\n",
        "lower case and other letters": b">a\n" + t.lower() + b"\n>b\nNNNN" + t + b"RYKM\n",
        "names": b">\n" + t + b"\n> lead\n" + t + b"\n>n2\twith tab\n" + t + b"\n>n3 some words\r\n" + t + b"\r\n>" + b"L" * 300 + b" x\n" + t + b"\n",
    }
    for w in (1, 15, 16, 17, 60, 61):
        reads = [t * 3, b"ACGT" * 40, (t * 4)[:97]]
        cases["width %d" % w] = reads_text(reads, w)
        cases["width %d crlf" % w] = reads_text(reads, w, b"\r\n")
    return cases


# -------------------------------------------------------------------------------------------- the library through ctypes
class Chunk(F.Chunk):
    """A ts_chunk fed with plain text, the FASTA walk over it (tests/fastachunk.py) and the read subset's three stages."""

    def reads_stage(self, records, at_end, batch, stream=None):
        return self.L.ts_fasta_chunk_stage(self.ptr, F.table_of(records), len(records), 1 if at_end else 0, batch, stream)

    def reads_gather(self, records, d_pass, cap, stream=None, fill=0xA5):
        """-> (rc, host_out as the call left it: cap bytes prefilled with `fill`, *bytes, *n_passed)"""
        out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
        nbytes, npassed = C.c_uint64(0xdead), C.c_uint64(0xdead)
        rc = self.L.ts_fasta_chunk_gather(self.ptr, F.table_of(records), len(records), d_pass, out, cap, C.byref(nbytes),
                                          C.byref(npassed), stream)
        return rc, (out.raw if cap else b""), nbytes.value, npassed.value

    def reads_block_lines(self, records, batch, cap, stream=None, fill=0x5A):
        """-> (rc, host_out as the call left it, *bytes, *n_lines)"""
        out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
        nbytes, nlines = C.c_uint64(0xdead), C.c_uint64(0xdead)
        rc = self.L.ts_fasta_chunk_block_lines(self.ptr, F.table_of(records), len(records), batch, out, cap, C.byref(nbytes),
                                               C.byref(nlines), stream)
        return rc, (out.raw if cap else b""), nbytes.value, nlines.value
