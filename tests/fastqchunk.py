"""What tests/test_fastq_chunk_reference_cpu.py, tests/test_gpu_fastq_chunk.py and tests/test_gpu_fastq_device.py share: a
plain-Python sequential restatement of the FASTQ walk (ref_walk) with its error kinds, references of the stage and the gather,
seeded generators of FASTQ text with their edge and error cases, and thin ctypes wrappers over ts_chunk_upload and the
ts_fastq_chunk_* entry points.  No test functions live here.

ref_walk restates the host route (fastqSubset in include/teloscope_mi355x_io.hpp, itself readFastqRecord of the reference), not
the kernels: it reads a line, skips it when blank in front of a header, takes three more lines whatever they hold, and checks
the record in the host route's order.  The device does the same by a prefix scan over line maps."""
import ctypes as C
import random

from tests import bamchunk as B

OK, TRUNCATED, BAD_HEADER, BAD_SEPARATOR, BAD_LENGTHS = 0, 1, 2, 3, 4
MESSAGES = {TRUNCATED: "truncated FASTQ record", BAD_HEADER: "expected header line starting with '@'",
            BAD_SEPARATOR: "expected separator line starting with '+'", BAD_LENGTHS: "sequence and quality length differ"}


# ------------------------------------------------------------------------------------------------------------ references
def ref_walk(text, at_end):
    """-> (records, next, error, error_record, error_off); a record is (off, seq_at, seq_len, size, seq_cr) as
    ts_fastq_record holds it.  at_end: the input ends with `text` (its last line may lack the newline); otherwise an unfinished line, and the
    record it belongs to, are left for the next chunk: `next` is where that chunk's carry starts."""
    text = bytes(text)
    n = len(text)

    def line(p):                                    # -> (begin, end without the newline, start of the next line) or None
        if p >= n:
            return None
        nl = text.find(b"\n", p)
        if nl < 0:
            return (p, n, n) if at_end else None
        return p, nl, nl + 1

    def logical(b, e):
        return e - b - 1 if e > b and text[e - 1] == 13 else e - b

    recs, pos = [], 0
    while True:
        h = line(pos)
        if h is None:
            break
        if logical(h[0], h[1]) == 0:                # a blank line in front of a header
            pos = h[2]
            continue
        s = line(h[2])
        p = line(s[2]) if s else None
        q = line(p[2]) if p else None
        if q is None:
            if at_end:
                return recs, h[0], TRUNCATED, len(recs), h[0]
            return recs, h[0], OK, 0, 0             # the record continues in the next chunk
        if text[h[0]] != 64:
            return recs, h[0], BAD_HEADER, len(recs), h[0]
        if p[1] == p[0] or text[p[0]] != 43:
            return recs, h[0], BAD_SEPARATOR, len(recs), h[0]
        if logical(s[0], s[1]) != logical(q[0], q[1]):
            return recs, h[0], BAD_LENGTHS, len(recs), h[0]
        recs.append((h[0], s[0] - h[0], s[1] - s[0], q[1] - h[0], s[1] - s[0] - logical(s[0], s[1])))
        pos = q[2]
    return recs, pos, OK, 0, 0


def ref_sequence(text, rec):
    """The bases the filter judges: the sequence line without its '\\r'."""
    off, seq_at, seq_len, _, seq_cr = rec
    return bytes(text[off + seq_at:off + seq_at + seq_len - seq_cr])


def ref_gather(text, recs, pass_bytes):
    """-> (the passing records' four lines and a newline behind each, in input order; how many they are)"""
    kept = [bytes(text[r[0]:r[0] + r[3]]) + b"\n" for r, p in zip(recs, pass_bytes) if p]
    return b"".join(kept), len(kept)


def ref_subset(text, read_filter):
    """The whole route on a complete text: (stdout bytes, kept, total) or raises ValueError with the host route's message."""
    if not text:
        raise ValueError("FASTQ input is empty")
    if text[:1] != b"@":
        raise ValueError("FASTQ input must start with '@'")
    recs, _, err, bad, _ = ref_walk(text, True)
    with_seq = [r for r in recs if r[2] > r[4]]
    passes = read_filter.filter([ref_sequence(text, r) for r in with_seq]) if with_seq else []
    out, kept = ref_gather(text, with_seq, passes)
    if err:
        raise ValueError("FASTQ record %d: %s" % (bad + 1, MESSAGES[err]))
    return out, kept, len(recs)


# ------------------------------------------------------------------------------------------------------------ generators
ALPHABET = b"ACGT"
QUALITIES = bytes(range(33, 127))                   # '@' and '+' among them: a quality line may begin with either


def random_read(gen, n, telomeric=False):
    if telomeric:
        unit = gen.choice((b"TTAGGG", b"CCCTAA"))
        return (unit * (n // 6 + 1))[:n]
    return bytes(gen.choice(ALPHABET) for _ in range(n))


def record_text(name, seq, qual=None, plus=b"+", eol=b"\n"):
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + plus + eol + qual + eol


def reads_text(seed, n_reads, lo=20, hi=400, eol=b"\n", every_telomeric=3):
    """n_reads well-formed records with every freedom the format leaves: quality lines that begin with '@' or '+', a '+'
    line that repeats the name, blank and "\\r" lines in front of headers, an empty sequence with an empty quality line."""
    gen = random.Random(seed)
    out = []
    for i in range(n_reads):
        n = 0 if i % 41 == 17 else gen.randrange(lo, hi)
        seq = random_read(gen, n, telomeric=i % every_telomeric == 0)
        qual = bytes(gen.choice(QUALITIES) for _ in range(n))
        if n and i % 5 == 1:
            qual = b"@" + qual[1:]
        if n and i % 5 == 3:
            qual = b"+" + qual[1:]
        name = b"r%d/%d some text" % (seed, i)
        plus = b"+" + name if i % 4 == 2 else b"+"
        if i % 13 == 5:
            out.append(b"\n")
        if i % 17 == 9:
            out.append(b"\r\n\n")
        out.append(record_text(name, seq, qual, plus, eol))
    return b"".join(out)


def edge_cases():
    """name -> complete text, every one well-formed."""
    a = record_text(b"a", b"TTAGGG" * 8)
    b = record_text(b"b", b"ACGT" * 9, qual=b"@" + b"+" * 35)
    c = record_text(b"c", b"CCCTAA" * 7, qual=b"+" + b"@" * 41, plus=b"+c")
    empty = record_text(b"none", b"", qual=b"")
    crlf = record_text(b"w", b"TTAGGG" * 9, eol=b"\r\n")
    return {
        "quality begins with @ and +": a + b + c + a,
        "plus repeats the name": c + c,
        "blank lines before headers": a + b"\n\n" + a + b"\n" + b + b"\r\n\r\n\n" + c,
        "blank lines only behind the last record": a + b"\n\r\n\n",
        "empty sequence and quality": a + empty + b + empty,
        "crlf": crlf + crlf + a + crlf,
        "no final newline": a + b + c[:-1],
        "no final newline, crlf": a + crlf[:-2],
        "no final newline, only the cr": a + crlf[:-1],
        "one record": a,
        "sequence of a lone cr": record_text(b"x", b"\r", qual=b"\r") + a,
        "generated": reads_text(3, 200),
        "generated crlf": reads_text(4, 120, eol=b"\r\n"),
    }


def _damage(kind, name):
    """One record that fails with `kind` (a truncated one is cut by the caller)."""
    good = record_text(name, b"TTAGGG" * 6)
    if kind == BAD_HEADER:
        return b"X" + good[1:]
    if kind == BAD_SEPARATOR:
        return good.replace(b"\n+\n", b"\n-\n", 1)
    if kind == BAD_LENGTHS:
        return good[:-2] + b"\n"
    return good


def error_cases():
    """name -> (complete text, error kind, index of the record it is reported for): each kind at the first, a middle and the
    last record (a truncated record can only be the last), an empty separator, and two errors in one text."""
    gen = random.Random(11)
    good = [record_text(b"g%d" % i, random_read(gen, 30 + i, telomeric=i % 2 == 0)) for i in range(9)]
    cases = {}
    for kind in (BAD_HEADER, BAD_SEPARATOR, BAD_LENGTHS):
        for where, at in (("first", 0), ("middle", 4), ("last", 8)):
            recs = list(good)
            recs[at] = _damage(kind, b"bad")
            text = b"".join(recs)
            if kind == BAD_HEADER and at == 0:
                text = good[0] + text                       # (a text that does not start with '@' is refused before any record)
                at = 1
            cases["%s at the %s record" % (MESSAGES[kind], where)] = (text, kind, at)
    for lines in (1, 2, 3):
        cut = b"\n".join(good[8].split(b"\n")[:lines])
        cases["truncated after %d lines" % lines] = (b"".join(good[:8]) + cut, TRUNCATED, 8)
        cases["truncated after %d lines and a newline" % lines] = (b"".join(good[:8]) + cut + b"\n", TRUNCATED, 8)
    cases["only a header"] = (b"@lonely", TRUNCATED, 0)
    # (getline finds no fourth line behind "+\n" at the end of the input: an empty quality line needs its newline)
    cases["empty quality line without its newline"] = (good[0] + b"@none\n\n+\n", TRUNCATED, 1)
    cases["empty separator"] = (good[0] + good[1].replace(b"\n+\n", b"\n\n", 1) + good[2], BAD_SEPARATOR, 1)
    cases["separator of a lone cr"] = (good[0] + good[1].replace(b"\n+\n", b"\n\r\n", 1) + good[2], BAD_SEPARATOR, 1)
    two = list(good)
    two[2] = _damage(BAD_LENGTHS, b"bad2")
    two[6] = _damage(BAD_HEADER, b"bad6")
    cases["two errors: the lower one"] = (b"".join(two), BAD_LENGTHS, 2)
    two = list(good)
    two[3] = _damage(BAD_SEPARATOR, b"bad3")
    cases["an error and a truncated end: the lower one"] = (b"".join(two)[:-20], BAD_SEPARATOR, 3)
    # a header-less line shifts the frame: four lines are taken whatever they hold
    cases["a stray line shifts the frame"] = (good[0] + b"stray\n" + good[1] + good[2], BAD_HEADER, 1)
    return cases


# -------------------------------------------------------------------------------------------- the library through ctypes
def table_of(records):
    from teloscope_amd import _capi as K
    arr = (K.FastqRecord * max(1, len(records)))()
    for i, (off, seq_at, seq_len, size, seq_cr) in enumerate(records):
        arr[i].off, arr[i].seq_at, arr[i].seq_len, arr[i].size, arr[i].seq_cr = off, seq_at, seq_len, size, seq_cr
    return arr


class Chunk(B.Chunk):
    """A ts_chunk fed with plain text or with BGZF members (B.Chunk.fill), and the FASTQ stages over it."""

    def reset(self):
        """Nothing held: the whole of what the chunk holds is dropped."""
        assert self.L.ts_chunk_upload(self.ptr, None, 0, self.size(), None) == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        self.mirror = b""
        assert self.size() == 0

    def upload(self, text, carry_from=None, stream=None):
        """The chunk's next contents: its tail from carry_from (default: nothing is carried), then `text`; the chunk must
        read back as exactly those bytes."""
        carry_from = len(self.mirror) if carry_from is None else carry_from
        rc = self.L.ts_chunk_upload(self.ptr, bytes(text), len(text), carry_from, stream)
        assert rc == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        self.mirror = self.mirror[carry_from:] + bytes(text)
        assert self.size() == len(self.mirror)
        assert self.read(0, len(self.mirror)) == self.mirror
        return self.mirror

    def fastq_walk(self, at_end, cap=1 << 16):
        """-> (records as tuples, next, error, error_record, error_off); what lies behind the records taken must be as it was."""
        K = self.K
        arr = (K.FastqRecord * (cap + 1))()
        C.memset(arr, 0xEE, C.sizeof(arr))
        n, nxt, err, erec, eoff = C.c_uint64(7), C.c_uint64(7), C.c_int(7), C.c_uint64(7), C.c_uint64(7)
        rc = self.L.ts_fastq_chunk_walk(self.ptr, 1 if at_end else 0, arr, cap, C.byref(n), C.byref(nxt), C.byref(err),
                                        C.byref(erec), C.byref(eoff))
        assert rc == K.TS_OK, self.L.ts_last_error(self.ctx)
        assert n.value <= cap
        recs = []
        for i in range(n.value):
            recs.append((arr[i].off, arr[i].seq_at, arr[i].seq_len, arr[i].size, arr[i].seq_cr))
        rest = bytes(arr)[n.value * C.sizeof(K.FastqRecord):]
        assert rest == b"\xee" * len(rest), "the walk wrote behind the records it reported"
        return recs, nxt.value, err.value, erec.value, eoff.value

    def stage(self, records, batch, stream=None):
        return self.L.ts_fastq_chunk_stage(self.ptr, table_of(records), len(records), batch, stream)

    def fastq_gather(self, records, d_pass, cap, stream=None, fill=0xA5):
        """-> (rc, host_out as the call left it: cap bytes prefilled with `fill`, *bytes, *n_passed)"""
        out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
        nbytes, npassed = C.c_uint64(0xdead), C.c_uint64(0xdead)
        rc = self.L.ts_fastq_chunk_gather(self.ptr, table_of(records), len(records), d_pass, out, cap, C.byref(nbytes),
                                          C.byref(npassed), stream)
        return rc, (out.raw if cap else b""), nbytes.value, npassed.value
