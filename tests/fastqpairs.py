"""What tests/test_fastq_pairs_reference_cpu.py, tests/test_gpu_fastq_pairs_chunk.py and tests/test_gpu_fastq_pairs_device.py
share: a plain-Python statement of the rule of interleaved paired FASTQ (include/teloscan.h: "Interleaved paired FASTQ") over
tests/fastqchunk.py's record walk, the name cases the rule names, and writers of paired text.  No test functions live here.

The statement works on the whole text at once: no chunks, no batches, no carry."""
from tests import fastqchunk as F
from tests import readblocks as RB

UNPAIRED = "FASTQ input ends with an unpaired record"
EMPTY = "FASTQ input is empty"
NO_HEADER = "FASTQ input must start with '@'"
NOT_STAGED = 0xFFFFFFFF


def name_error(j):
    """Of pair j (counted from 0): the records are named from 1."""
    return "FASTQ records %d and %d do not have the same name" % (2 * j + 1, 2 * j + 2)


def record_error(kind, r):
    """Of record r (counted from 0)."""
    return "FASTQ record %d: %s" % (r + 1, F.MESSAGES[kind])


# ------------------------------------------------------------------------------------------------------------ the rule
def ref_name(text, rec):
    """The read block report's FASTQ name of a record of F.ref_walk."""
    off, seq_at = rec[0], rec[1]
    return RB.fastq_name(bytes(text[off:off + seq_at]))


def mate_name(name):
    """The name without one trailing "/1" or "/2"."""
    return name[:-2] if name[-2:] in (b"/1", b"/2") else name


def ref_mates(text, a, b):
    return mate_name(ref_name(text, a)) == mate_name(ref_name(text, b))


def ref_mismatch(text, recs):
    """The lowest j for which recs[2j] and recs[2j+1] are not mates, or None."""
    assert len(recs) % 2 == 0
    for j in range(len(recs) // 2):
        if not ref_mates(text, recs[2 * j], recs[2 * j + 1]):
            return j
    return None


def ref_pair_pass(read_of, passes):
    """Both bytes of a pair are 1 when either mate's own pass byte is set (read_of: the record's index in passes, or NOT_STAGED)."""
    own = [r != NOT_STAGED and passes[r] != 0 for r in read_of]
    out = bytearray()
    for j in range(len(own) // 2):
        out += bytes([1, 1]) if own[2 * j] or own[2 * j + 1] else bytes(2)
    return bytes(out)


def ref_paired_subset(text, read_filter):
    """The whole route on a complete text: (output bytes — what is written before the failure, when there is one; (total, kept):
    records read and records written; the message or None; [(name, bases)] of the written records that were judged, in output
    order: what tests/readblocks.py's ref_report makes the block report from)."""
    text = bytes(text)
    if not text:
        return b"", (0, 0), EMPTY, []
    if text[:1] != b"@":
        return b"", (0, 0), NO_HEADER, []
    recs, _, err, bad, _ = F.ref_walk(text, True)
    message = None
    pairs = len(recs) // 2                          # whole pairs of valid records: an odd one in front of a bad record is dropped
    if err:
        message = record_error(err, bad)
    elif len(recs) % 2:
        message = UNPAIRED
    j = ref_mismatch(text, recs[:2 * pairs])
    if j is not None:                               # a pair wholly in front of the bad record, or of the unpaired one: it wins
        message, pairs = name_error(j), j
    recs = recs[:2 * pairs]
    read_of, with_seq = [], []
    for r in recs:
        if r[2] > r[4]:
            read_of.append(len(with_seq))
            with_seq.append(r)
        else:
            read_of.append(NOT_STAGED)
    reads = [F.ref_sequence(text, r) for r in with_seq]
    passes = read_filter.filter(reads) if reads else []
    keep = ref_pair_pass(read_of, [1 if p else 0 for p in passes])
    out, kept = F.ref_gather(text, recs, keep)
    judged = [(ref_name(text, r), F.ref_sequence(text, r)) for r, k in zip(recs, keep) if k and r[2] > r[4]]
    total = 2 * pairs if message else len(recs)
    return out, (total, kept), message, judged


def figures(stats):
    total, kept = stats
    return "FASTQ paired subset: kept %d of %d records." % (kept, total)


# ------------------------------------------------------------------------------------------------------------ names
MATE_LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65)


def stem(n, salt=0):
    """A mate name of n bytes without '/', space or tab."""
    return bytes(97 + (i * 7 + salt) % 26 for i in range(n))


def name_cases():
    """[(first mate's name, second mate's name, whether they are mates, what)]: every length with no suffix, with /1 + /2 and with
    the suffix on one mate only; what is no suffix; names that differ in the first byte, the last byte or the length."""
    cases = []
    for n in MATE_LENGTHS:
        s = stem(n, n)
        cases.append((s, s, True, "length %d, bare" % n))
        cases.append((s + b"/1", s + b"/2", True, "length %d, /1 and /2" % n))
        cases.append((s + b"/1", s, True, "length %d, suffix on the first" % n))
        cases.append((s, s + b"/2", True, "length %d, suffix on the second" % n))
        if n:
            cases.append((bytes([s[0] ^ 1]) + s[1:], s, False, "length %d, first byte differs" % n))
            cases.append((s + b"/1", s[:-1] + bytes([s[-1] ^ 1]) + b"/2", False, "length %d, last byte differs" % n))
            cases.append((s, s + b"x", False, "length %d against %d" % (n, n + 1)))
    cases += [
        (b"a/3", b"a", False, "/3 is no suffix"), (b"a/3", b"a/3", True, "/3 stays"), (b"a/12", b"a/1", False, "/12 is no suffix"),
        (b"a/12", b"a/12", True, "/12 stays"), (b"a/1/1", b"a/1", False, "a/1/1 against a/1: the suffix is removed once from each"),
        (b"a/1/1", b"a", False, "the suffix is removed once"), (b"a/1/1", b"a/1/2", True, "a/1 is the mate name"), (b"a/1/", b"a", False, "/1/ is no suffix"), (b"a/1/", b"a/1/", True, "/1/ stays"),
        (b"/1", b"", True, "a name of exactly /1 is empty"), (b"/1", b"/2", True, "two suffixes alone"), (b"/", b"", False, "a lone slash"),
        (b"1", b"2", False, "digits alone"), (b"a/2", b"a/2", True, "two second mates"), (b"a/0", b"a", False, "/0 is no suffix"),
    ]
    return cases


# ------------------------------------------------------------------------------------------------------------ writers
def pair_text(name_a, name_b, seq_a, seq_b, eol=b"\n", end_a=b"", end_b=b""):
    """A pair: end_a / end_b stand behind the names in the header lines (b" 1:N:0", b"\\tx")."""
    return F.record_text(name_a + end_a, seq_a, eol=eol) + F.record_text(name_b + end_b, seq_b, eol=eol)


STYLES = ("slash", "comment", "bare")


def pair_names(j, style):
    """-> (first header behind '@', second header behind '@')"""
    if style == "slash":
        return b"p%d/1" % j, b"p%d/2" % j
    if style == "comment":
        return b"p%d 1:N:0" % j, b"p%d 2:N:0" % j
    return b"p%d" % j, b"p%d" % j


def paired_text(reads, style, eol=b"\n"):
    """The reads in their order as pairs (reads 2j and 2j+1 are pair j), named in `style`."""
    assert len(reads) % 2 == 0
    out = []
    for j in range(len(reads) // 2):
        a, b = pair_names(j, style)
        out.append(F.record_text(a, reads[2 * j], eol=eol) + F.record_text(b, reads[2 * j + 1], eol=eol))
    return b"".join(out)


# -------------------------------------------------------------------------------------------- the library through ctypes
def chunk_mates(chunk, records):
    """ts_fastq_chunk_mates over a tests/fastqchunk.py Chunk -> (rc, *mismatch; 7 where the call left it alone)"""
    import ctypes as C
    mismatch = C.c_uint64(7)
    rc = chunk.L.ts_fastq_chunk_mates(chunk.ptr, F.table_of(records), len(records), C.byref(mismatch))
    return rc, mismatch.value


def chunk_pair_pass(chunk, read_of, d_pass, d_pair_pass, stream=None):
    import ctypes as C
    arr = (C.c_uint32 * max(1, len(read_of)))(*read_of)
    return chunk.L.ts_fastq_chunk_pair_pass(chunk.ptr, len(read_of), arr, d_pass, d_pair_pass, stream)
