"""What tests/test_sam_chunk_reference_cpu.py, tests/test_gpu_sam_chunk.py and tests/test_gpu_sam_device.py share: a plain-Python
sequential restatement of the SAM rule of include/teloscan.h (ref_walk) with its error kinds, references of the stage and the
gather and of the whole route, seeded generators of SAM text with their edge and error cases, a BAM -> SAM conversion, and thin
ctypes wrappers over the ts_sam_chunk_* entry points.  No test functions live here.

ref_walk restates the rule, not the kernels: it reads a line, decides header or alignment by its first byte, splits an alignment
line at its tabs and applies the checks in the rule's order, and stops at the first line that fails one.  The device does the
same with a lane per line over the chunk layer's line and tab indexes."""
import ctypes as C
import random
import struct

from tests import fastqchunk as F

OK, HEADER_AFTER_RECORD, TOO_FEW_FIELDS, EMPTY_SEQ, BAD_LENGTHS = 0, 1, 2, 3, 4
MESSAGES = {HEADER_AFTER_RECORD: "header line after the first alignment record", TOO_FEW_FIELDS: "fewer than 11 fields",
            EMPTY_SEQ: "empty SEQ field", BAD_LENGTHS: "SEQ and QUAL length differ"}
SEQ_IS_STAR = 1


# ------------------------------------------------------------------------------------------------------------ references
def lines_of(text, at_end):
    """-> [(begin, end of the content, end of the line without its newline, start of the next line)] of the whole lines."""
    out, p, n = [], 0, len(text)
    while p < n:
        nl = text.find(b"\n", p)
        if nl < 0:
            if not at_end:
                break
            nl, nxt = n, n
        else:
            nxt = nl + 1
        e = nl - 1 if nl > p and text[nl - 1] == 13 else nl
        out.append((p, e, nl, nxt))
        p = nxt
    return out


def ref_line(text, b, e, line_end):
    """An alignment line with content text[b:e] -> (error, record): a record is (off, seq_at, seq_len, size, flags) as
    ts_sam_record holds it."""
    fields = bytes(text[b:e]).split(b"\t")
    if len(fields) < 11:
        return TOO_FEW_FIELDS, None
    seq, qual = fields[9], fields[10]
    seq_at = sum(len(f) + 1 for f in fields[:9])
    rec = (b, seq_at, len(seq), line_end - b, SEQ_IS_STAR if seq == b"*" else 0)
    if len(seq) == 0:
        return EMPTY_SEQ, rec
    if seq != b"*" and qual != b"*" and len(seq) != len(qual):
        return BAD_LENGTHS, rec
    return OK, rec


def ref_walk(text, at_end, in_header):
    """-> (records, n_header_lines, header_end, n_lines, next, error, error_line, error_off), with the meanings
    ts_sam_chunk_walk gives them."""
    text = bytes(text)
    recs, headers, header_end, header = [], 0, 0, bool(in_header)
    lines = lines_of(text, at_end)
    nxt = lines[-1][3] if lines else 0
    for i, (b, e, line_end, _) in enumerate(lines):
        if text[b:b + 1] == b"@" and line_end > b:
            if not header:
                return recs, headers, header_end, i, b, HEADER_AFTER_RECORD, i, b
            headers += 1
            continue
        if header:
            header, header_end = False, b
        err, rec = ref_line(text, b, e, line_end)
        if err:
            return recs, headers, header_end, i, b, err, i, b
        recs.append(rec)
    if header:
        header_end = nxt
    return recs, headers, header_end, len(lines), nxt, OK, 0, 0


def ref_sequence(text, rec):
    off, seq_at, seq_len, _, _ = rec
    return bytes(text[off + seq_at:off + seq_at + seq_len])


def ref_gather(text, recs, pass_bytes):
    """-> (the passing records' lines and a newline behind each, in input order; how many they are)"""
    kept = [bytes(text[r[0]:r[0] + r[3]]) + b"\n" for r, p in zip(recs, pass_bytes) if p]
    return b"".join(kept), len(kept)


def ref_subset(text, read_filter):
    """The whole route on a complete text: (stdout bytes, (header lines, total, kept, without sequence), message or None); the
    message is the exception's text, and the bytes are then what is written before it."""
    if not text:
        return b"", (0, 0, 0, 0), "SAM input is empty"
    recs, headers, header_end, _, _, err, bad, _ = ref_walk(text, True, True)
    with_seq = [r for r in recs if not r[4] & SEQ_IS_STAR]
    passes = read_filter.filter([ref_sequence(text, r) for r in with_seq]) if with_seq else []
    out, kept = ref_gather(text, with_seq, passes)
    msg = "SAM line %d: %s" % (bad + 1, MESSAGES[err]) if err else None
    return bytes(text[:header_end]) + out, (headers, len(recs), kept, len(recs) - len(with_seq)), msg


def kept_names(out):
    """QNAMEs of the alignment lines of a subset."""
    return [l.split(b"\t")[0].decode() for l in out.split(b"\n") if l and not l.startswith(b"@")]


# ------------------------------------------------------------------------------------------------------------ generators
HEADER = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@PG\tID:gen\tCL:a\tb c\n@CO\tfree text, no tabs\n"


def sam_line(name, seq, qual=None, tags=(), flag=4, eol=b"\n"):
    qual = b"I" * len(seq) if qual is None else qual
    fields = [name, b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, qual] + list(tags)
    return b"\t".join(fields) + eol


def reads_text(reads, header=HEADER, eol=b"\n", seed=1):
    """The reads as unmapped alignment lines r0, r1, ... behind `header`: trailing tags on some, QUAL "*" on some, and some
    records without sequence in between (named s<i>)."""
    gen = random.Random(seed)
    out = [header.replace(b"\n", eol)]
    for i, r in enumerate(reads):
        tags = [(), (b"NM:i:0",), (b"RG:Z:x", b"XS:A:+", b"ZZ:Z:" + b"t" * gen.randrange(1, 40))][i % 3]
        qual = b"*" if i % 7 == 2 else bytes(gen.choice(F.QUALITIES) for _ in range(len(r)))
        out.append(sam_line(b"r%d" % i, r, qual, tags, eol=eol))
        if i % 11 == 4:
            out.append(sam_line(b"s%d" % i, b"*", b"*", tags, eol=eol))
    return b"".join(out)


def generated(seed, n_reads, lo=1, hi=300, eol=b"\n", header=HEADER):
    gen = random.Random(seed)
    reads = [F.random_read(gen, gen.randrange(lo, hi), telomeric=i % 3 == 0) for i in range(n_reads)]
    return reads_text(reads, header, eol, seed)


def edge_cases():
    """name -> complete text, every one well-formed."""
    a = sam_line(b"a", b"TTAGGG" * 8)
    b = sam_line(b"b", b"ACGT" * 9, tags=(b"NM:i:3", b"MD:Z:36"))
    star = sam_line(b"nothing", b"*", b"*")
    noqual = sam_line(b"noqual", b"CCCTAA" * 7, b"*")
    crlf = sam_line(b"w", b"TTAGGG" * 9, eol=b"\r\n")
    crlf_tags = sam_line(b"wt", b"TTAGGG" * 9, tags=(b"NM:i:0",), eol=b"\r\n")
    return {
        "header and records": HEADER + a + b + a,
        "no header": a + b,
        "header only": HEADER,
        "header only, no final newline": HEADER[:-1],
        "one header line, no newline": b"@CO",
        "one record": a,
        "trailing tags": b + b + sam_line(b"t", b"ACGT", tags=(b"X1:i:1",) * 30),
        "qual is the last field, with and without cr": a + crlf + a[:-1],
        "seq and qual are stars": HEADER + star + a + star,
        "seq present, qual star": noqual + a,
        "seq star, qual present": sam_line(b"odd", b"*", b"IIII") + a,
        "one base": sam_line(b"one", b"A") + sam_line(b"onestar", b"A", b"*"),
        "crlf": HEADER.replace(b"\n", b"\r\n") + crlf + crlf_tags + crlf,
        "no final newline": HEADER + a + b[:-1],
        "no final newline, crlf": a + crlf[:-2],
        "no final newline, only the cr": a + crlf[:-1],
        "empty qual field before a tag": sam_line(b"eq", b"*", b"", tags=(b"NM:i:0",)),
        "iupac and lower case": sam_line(b"i", b"ttagggTTAGGGNRYK=.TTAGGG" * 3),
        "generated": generated(3, 200),
        "generated crlf": generated(4, 120, eol=b"\r\n"),
    }


def error_cases():
    """name -> (complete text, error kind, line of the input it is reported for, counted from 0)."""
    gen = random.Random(11)
    good = [sam_line(b"g%d" % i, F.random_read(gen, 30 + i, telomeric=i % 2 == 0)) for i in range(9)]
    nine_tabs = b"\t".join([b"short", b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT"]) + b"\n"
    rich = sam_line(b"rich", b"ACGT", tags=(b"X1:i:1",) * 12)
    bad = {TOO_FEW_FIELDS: nine_tabs, EMPTY_SEQ: sam_line(b"e", b"", b""), BAD_LENGTHS: sam_line(b"l", b"ACGT", b"III"),
           HEADER_AFTER_RECORD: b"@CO\tlate\n"}
    cases = {}
    nh = HEADER.count(b"\n")
    for kind, line in bad.items():
        for where, at in (("first", 0), ("middle", 4), ("last", 8)):
            if kind == HEADER_AFTER_RECORD and at == 0:
                continue
            recs = list(good)
            recs[at] = line
            cases["%s at the %s record" % (MESSAGES[kind], where)] = (HEADER + b"".join(recs), kind, nh + at)
    cases["header after the only record"] = (good[0] + b"@HD\tVN:1.6\n", HEADER_AFTER_RECORD, 1)
    cases["a short line borrows no tab"] = (HEADER + good[0] + nine_tabs + rich + good[1], TOO_FEW_FIELDS, nh + 1)
    cases["exactly ten tabs, then nine"] = (sam_line(b"ten", b"ACGT") + nine_tabs + rich, TOO_FEW_FIELDS, 1)
    cases["an empty line"] = (HEADER + good[0] + b"\n" + good[1], TOO_FEW_FIELDS, nh + 1)
    cases["a line of a lone cr"] = (HEADER + good[0] + b"\r\n" + good[1], TOO_FEW_FIELDS, nh + 1)
    cases["an empty line at the end"] = (good[0] + b"\n", TOO_FEW_FIELDS, 1)
    cases["an empty first line"] = (b"\n" + HEADER, TOO_FEW_FIELDS, 0)
    cases["empty seq before tags"] = (good[0] + sam_line(b"e", b"", b"*", tags=(b"NM:i:0",)), EMPTY_SEQ, 1)
    cases["unequal lengths, crlf"] = (good[0] + sam_line(b"l", b"ACGT", b"IIIII", eol=b"\r\n"), BAD_LENGTHS, 1)
    cases["unequal lengths, no final newline"] = (good[0] + sam_line(b"l", b"ACGT", b"II")[:-1], BAD_LENGTHS, 1)
    cases["unequal lengths, qual empty"] = (good[0] + sam_line(b"l", b"ACGT", b""), BAD_LENGTHS, 1)
    two = list(good)
    two[2] = bad[BAD_LENGTHS]
    two[6] = bad[TOO_FEW_FIELDS]
    cases["two errors: the lower one"] = (HEADER + b"".join(two), BAD_LENGTHS, nh + 2)
    two = list(good)
    two[3] = bad[HEADER_AFTER_RECORD]
    two[5] = bad[EMPTY_SEQ]
    cases["a late header and a bad record: the lower one"] = (b"".join(two), HEADER_AFTER_RECORD, 3)
    return cases


# -------------------------------------------------------------------------------------------------------- BAM -> SAM
def bam_to_sam(plain):
    """An uncompressed BAM (header, references, records) as SAM text, field by field as samtools view -h writes them."""
    assert plain[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", plain, 4)
    out = [bytes(plain[8:8 + l_text]).rstrip(b"\0")]
    pos = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", plain, pos)
    pos += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", plain, pos)
        refs.append(bytes(plain[pos + 4:pos + 4 + l_name - 1]))
        pos += 4 + l_name + 4
    while pos < len(plain):
        (bs,) = struct.unpack_from("<i", plain, pos)
        ref, p, l_name, mapq, _, n_cigar, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", plain, pos + 4)
        at = pos + 36
        name = bytes(plain[at:at + l_name - 1])
        at += l_name
        cigar = b"".join(b"%d%c" % (v >> 4, b"MIDNSHP=X"[v & 15]) for v in struct.unpack_from("<%dI" % n_cigar, plain, at))
        at += 4 * n_cigar
        packed = plain[at:at + (l_seq + 1) // 2]
        seq = bytes(b"=ACMGRSVTWYHKDBN"[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        at += (l_seq + 1) // 2
        q = bytes(plain[at:at + l_seq])
        qual = b"*" if l_seq == 0 or q == b"\xff" * l_seq else bytes(c + 33 for c in q)
        rname = refs[ref] if ref >= 0 else b"*"
        rnext = b"*" if nref < 0 else b"=" if nref == ref else refs[nref]
        fields = [name, b"%d" % flag, rname, b"%d" % (p + 1), b"%d" % mapq, cigar or b"*", rnext, b"%d" % (npos + 1), b"%d" % tlen,
                  seq or b"*", qual]
        out.append(b"\t".join(fields) + b"\n")
        pos += 4 + bs
    return b"".join(out)


# -------------------------------------------------------------------------------------------- the library through ctypes
def table_of(records):
    from teloscope_amd import _capi as K
    arr = (K.SamRecord * max(1, len(records)))()
    for i, (off, seq_at, seq_len, size, flags) in enumerate(records):
        arr[i].off, arr[i].seq_at, arr[i].seq_len, arr[i].size, arr[i].flags = off, seq_at, seq_len, size, flags
    return arr


class Chunk(F.Chunk):
    """A ts_chunk fed with plain text (F.Chunk.upload) or with BGZF members (B.Chunk.fill), and the SAM stages over it."""

    def sam_walk_raw(self, at_end, in_header, cap):
        K = self.K
        arr = (K.SamRecord * (cap + 1))()
        C.memset(arr, 0xEE, C.sizeof(arr))
        w = [C.c_uint64(7) for _ in range(5)]                       # n, n_header_lines, header_end, n_lines, next
        err, eline, eoff = C.c_int(7), C.c_uint64(7), C.c_uint64(7)
        rc = self.L.ts_sam_chunk_walk(self.ptr, 1 if at_end else 0, 1 if in_header else 0, arr, cap, *[C.byref(x) for x in w],
                                      C.byref(err), C.byref(eline), C.byref(eoff))
        return rc, arr, [x.value for x in w], (err.value, eline.value, eoff.value)

    def sam_walk(self, at_end, in_header, cap=1 << 16):
        """-> ref_walk's tuple; what lies behind the records taken must be as it was."""
        K = self.K
        rc, arr, (n, headers, header_end, n_lines, nxt), (err, eline, eoff) = self.sam_walk_raw(at_end, in_header, cap)
        assert rc == K.TS_OK, self.L.ts_last_error(self.ctx)
        assert n <= cap
        recs = [(arr[i].off, arr[i].seq_at, arr[i].seq_len, arr[i].size, arr[i].flags) for i in range(n)]
        rest = bytes(arr)[n * C.sizeof(K.SamRecord):]
        assert rest == b"\xee" * len(rest), "the walk wrote behind the records it reported"
        return recs, headers, header_end, n_lines, nxt, err, eline, eoff

    def sam_stage(self, records, batch, stream=None):
        return self.L.ts_sam_chunk_stage(self.ptr, table_of(records), len(records), batch, stream)

    def sam_gather(self, records, d_pass, cap, stream=None, fill=0xA5):
        """-> (rc, host_out as the call left it: cap bytes prefilled with `fill`, *bytes, *n_passed)"""
        out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
        nbytes, npassed = C.c_uint64(0xdead), C.c_uint64(0xdead)
        rc = self.L.ts_sam_chunk_gather(self.ptr, table_of(records), len(records), d_pass, out, cap, C.byref(nbytes),
                                        C.byref(npassed), stream)
        return rc, (out.raw if cap else b""), nbytes.value, npassed.value
