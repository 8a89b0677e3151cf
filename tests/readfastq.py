"""FASTQ out of the BAM and SAM subsets in plain Python (include/teloscan.h: "FASTQ out of the BAM and SAM subsets"), for the tests
of its device and host forms: the rule restated from the header's text, and builders of BAM records and SAM lines with a chosen
name, FLAG, SEQ and QUAL.  Nothing here calls the library under test."""
import struct

RESTORE_STRAND = 1
BAM_LETTERS = b"=ACMGRSVTWYHKDBN"
BAM_CODE = {c: i for i, c in enumerate(BAM_LETTERS)}
_PAIRS = {b"A": b"T", b"C": b"G", b"M": b"K", b"R": b"Y", b"V": b"B", b"H": b"D"}
SAM_COMP = {}
for _a, _b in _PAIRS.items():
    for _x, _y in ((_a, _b), (_b, _a)):
        SAM_COMP[_x[0]] = _y[0]
        SAM_COMP[_x.lower()[0]] = _y.lower()[0]
SAM_COMP[ord("U")] = ord("A")
SAM_COMP[ord("u")] = ord("a")


def rev4(code):
    return ((code & 1) << 3) | ((code & 2) << 1) | ((code & 4) >> 1) | ((code & 8) >> 3)


def text_of(name, bases, quals):
    return b"@" + name + b"\n" + bases + b"\n+\n" + quals + b"\n"


# ---- BAM

def bam_record(name, flag, codes, qual, n_cigar=0, tail=b""):
    """A BAM record from its block_size field on.  codes: one 4-bit code per base; qual: bytes of len(codes) (raw Phred), or None
    for a missing QUAL (0xFF bytes).  tail: tag bytes behind QUAL."""
    a = list(codes) + [0]
    seq = bytes((a[j] << 4) | a[j + 1] for j in range(0, len(codes), 2))
    q = b"\xff" * len(codes) if qual is None else bytes(qual)
    assert len(q) == len(codes)
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, n_cigar, flag, len(codes), -1, -1, 0) + name + b"\0" + \
        b"\x10\x00\x00\x00" * n_cigar + seq + q + tail
    return struct.pack("<I", len(body)) + body


def bam_codes(bases):
    """ASCII bases -> codes, as a BAM writer maps them (anything that is no letter of the table: N)"""
    return [BAM_CODE.get(c, 15) for c in bases.upper()]


def bam_text(rec, flags):
    """The rule on a BAM record (bytes from its block_size field on)."""
    l_read_name = rec[12]
    n_cigar, flag, l_seq = struct.unpack_from("<HHi", rec, 16)
    assert struct.unpack_from("<H", rec, 18)[0] == flag
    name = rec[36:36 + l_read_name - 1]
    at = 36 + l_read_name + 4 * n_cigar
    packed = rec[at:at + (l_seq + 1) // 2]
    codes = [(packed[i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
    raw = rec[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq]
    quals = b"!" * l_seq if raw[:1] == b"\xff" else bytes(min(q, 93) + 33 for q in raw)
    if (flags & RESTORE_STRAND) and (flag & 0x10):
        codes = [rev4(c) for c in reversed(codes)]
        quals = quals[::-1]
    return text_of(name, bytes(BAM_LETTERS[c] for c in codes), quals)


# ---- SAM

def sam_line(name, flag_field, seq, qual, tags=None, eol=b"\n"):
    """An alignment line: flag_field is field 2's bytes as they are; qual b"*" is a missing QUAL; tags: bytes behind a tab, or None."""
    fields = [name, flag_field, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, qual]
    return b"\t".join(fields) + (b"\t" + tags if tags is not None else b"") + eol


def sam_flag(field):
    v = 0
    for c in field[:9]:
        if not 48 <= c <= 57:
            break
        v = v * 10 + c - 48
    return v


def sam_text(line, flags):
    """The rule on a SAM alignment line (with or without its line end)."""
    content = line[:-1] if line.endswith(b"\n") else line
    if content.endswith(b"\r"):
        content = content[:-1]
    f = content.split(b"\t")
    name, seq, qual = f[0], f[9], f[10]
    quals = b"!" * len(seq) if qual == b"*" else qual
    assert len(quals) == len(seq)
    bases = seq
    if (flags & RESTORE_STRAND) and (sam_flag(f[1]) & 0x10):
        bases = bytes(SAM_COMP.get(c, c) for c in reversed(seq))
        quals = quals[::-1]
    return text_of(name, bases, quals)


# ---- a FASTQ written as BAM and as SAM, for the round trip through the routes

def comp_ascii(bases):
    return bytes(SAM_COMP.get(c, c) for c in reversed(bases))


def fastq_as_bam_records(records, reverse):
    """records: [(name, bases over ACGTN, quals as Phred+33 bytes)] -> BAM records; reverse: FLAG 16, SEQ and QUAL stored reversed"""
    out = []
    for name, bases, quals in records:
        b, q = (comp_ascii(bases), quals[::-1]) if reverse else (bases, quals)
        out.append(bam_record(name, 16 if reverse else 4, bam_codes(b), bytes(c - 33 for c in q)))
    return b"".join(out)


def fastq_as_sam(records, reverse):
    out = []
    for name, bases, quals in records:
        b, q = (comp_ascii(bases), quals[::-1]) if reverse else (bases, quals)
        out.append(sam_line(name, b"16" if reverse else b"4", b, q))
    return b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(out)


def bam_header():
    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
