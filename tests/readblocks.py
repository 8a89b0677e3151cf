"""The read block report in plain Python (include/teloscan.h: "The read block report"), for the tests of its device and host
forms: one line per terminal block of every kept read, from the CPU oracle's blocks of the read scanned as one tips-only segment
at abs_pos 0 under the read filter's parameters.  Nothing here calls the library under test."""
import functools
import struct
import zlib

from tests import readsets as R

MASK64 = (1 << 64) - 1


def read_oracle(flags):
    """The oracle a ReadTelomereFilter of these options scans with (tests/backends.py: OracleReadFilter)."""
    from tests.backends import OracleReadFilter
    return OracleReadFilter(R.options(flags)).oracle


def label_byte(v):
    return v if isinstance(v, bytes) else bytes([int(v)])


def block_rows(oracle, seq):
    """[(start, block_len, label, forward, reverse, canonical, non_canonical)] of the read's terminal blocks, in the oracle's order."""
    tb = oracle.scan_segment(seq, 0, tips_only=True)["terminal_blocks"]
    return [(int(b["start"]), int(b["block_len"]), label_byte(b["block_label"]), int(b["forward_count"]), int(b["reverse_count"]),
             int(b["canonical_count"]), int(b["non_canonical_count"])) for b in tb]


def format_line(name, row, read_len):
    start, block_len, label, fwd, rev, can, noncan = row
    return name + b"\t%d\t%d\t%d\t" % (start, (start + block_len) & MASK64, block_len) + label + b"\t%d\t%d\t%d\t%d\t%d\n" % (fwd, rev, can, noncan, read_len)


def fastq_name(header_line):
    """header_line: the record's first line with its line end."""
    content = header_line[:-1] if header_line.endswith(b"\n") else header_line
    if content.endswith(b"\r"):
        content = content[:-1]
    name = content[1:]
    for i, c in enumerate(name):
        if c in b" \t":
            return name[:i]
    return name


def sam_name(line):
    return line.split(b"\t", 1)[0]


def ref_report(records, oracle):
    """records: [(name, bases judged)] in output order, kept or not -> (the report's bytes, the names of the records with a
    line, in order)."""
    out, kept = [], []
    for name, seq in records:
        rows = block_rows(oracle, seq)
        if rows:
            kept.append(name)
        out.extend(format_line(name, row, len(seq)) for row in rows)
    return b"".join(out), kept


@functools.lru_cache(maxsize=None)
def set_report(flags):
    """ref_report of readsets.reads_for(flags) under the names readsets.fastq_records gives them."""
    reads = R.reads_for(flags)
    return ref_report([(b"r%d" % i, r) for i, r in enumerate(reads)], read_oracle(flags))


# ---- inputs of the three front ends over the same reads, with the names the report must print

def fastq_input(reads):
    """names of several shapes: a comment behind a space, behind a tab, an empty name, a '\\r' line end"""
    recs, names = [], []
    for i, r in enumerate(reads):
        name = b"" if i % 11 == 5 else b"read/%d" % i
        eol = b"\r\n" if i % 7 == 3 else b"\n"
        head = b"@" + name + (b" len=%d" % len(r) if i % 3 == 0 else b"\tx" if i % 3 == 1 else b"")
        recs.append(head + eol + r + eol + b"+" + eol + b"I" * len(r) + eol)
        names.append(name)
    return b"".join(recs), names


def sam_input(reads):
    lines, names = [], []
    for i, r in enumerate(reads):
        name = b"" if i % 11 == 5 else b"q%d:x y" % i
        lines.append(b"\t".join([name, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", r, b"*"]) + (b"\r\n" if i % 5 == 2 else b"\n"))
        names.append(name)
    return b"".join(lines), names


def bam_records(reads):
    code = {65: 1, 67: 2, 71: 4, 84: 8}
    recs, names = [], []
    for i, r in enumerate(reads):
        name = b"n" if i % 11 == 5 else b"bam_read_%d" % i
        a = [code.get(c, 15) for c in r] + [0]
        seq = bytes((a[j] << 4) | a[j + 1] for j in range(0, len(r), 2))
        flag = 0x900 if i % 4 == 1 else 4                        # (secondary + supplementary: a record like any other)
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, flag, len(r), -1, -1, 0) + name + b"\0" + seq + b"\xff" * len(r)
        recs.append(struct.pack("<I", len(body)) + body)
        names.append(name)
    return b"".join(recs), names


EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf(data, chunk=0xff00):
    out = []
    for a in range(0, len(data), chunk):
        piece = data[a:a + chunk]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(piece) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
                   struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    return b"".join(out) + EOF_BLOCK


def bam_file(reads, chunk=0xff00):
    """-> (a BAM of bam_records(reads), the names)"""
    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    header = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
    records, names = bam_records(reads)
    return bgzf(header + records, chunk), names
