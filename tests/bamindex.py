"""What tests/test_bam_index_cpu.py and tests/test_gpu_bam_index.py share: a plain-Python model of the parallel record index
(ts_bam_chunk_index: spans, candidates, chain, write), the inputs built for it (decoys, boundary and long records, short
reads), and the case file that tests/cpp/bam_index_host.cpp reads.  No test functions live here.

The model restates the scheme, not the code: a chunk is cut at absolute multiples of S; a span's candidates are its first K
offsets, ascending, from which the serial rule (tests/bamchunk.py: ref_walk's loop body) survives to the span's end; the chain
starts at `from`, takes a span's exit and record count from the row whose entry it stands on and otherwise walks that span by
the serial rule; the table is what the serial rule gives from each entered span's entry."""
import random
import struct

import numpy as np

from tests import bamchunk as B

SPAN_END, INCOMPLETE, SHORT = 0, 5, 6             # what ends a span's walk without an error (1 .. 4: ref_walk's error codes)
GEOMETRIES = [(s, k) for s in (64, 256, 1024) for k in (1, 4)]


def record_at(plain, pos):
    """The serial rule at pos -> (code, record): 0 and (off, block_size, seq_at, l_seq), or what stops the walk there."""
    n = len(plain)
    if n - pos < 4:
        return SHORT, None
    bs = struct.unpack_from("<i", plain, pos)[0]
    if bs < 32 or bs > B.MAX_BLOCK_SIZE:
        return 1, None
    if n - pos < 4 + bs:
        return INCOMPLETE, None
    lname, ncig = plain[pos + 12], struct.unpack_from("<H", plain, pos + 16)[0]
    lseq = struct.unpack_from("<I", plain, pos + 20)[0]
    seq_at = 32 + lname + 4 * ncig
    if lname == 0 or lseq > 0x7fffffff:
        return 2, None
    if seq_at + (lseq + 1) // 2 + lseq > bs:
        return 3, None
    if plain[pos + 36 + lname - 1] != 0:
        return 4, None
    return 0, (pos, bs, 4 + seq_at, lseq)


def span_walk(plain, entry, span_end, limit=1 << 62):
    """-> (exit, records, stop): the serial rule from entry until it stands at or beyond span_end, stops, or has `limit`."""
    pos, recs = entry, []
    while pos < span_end:
        if len(recs) == limit:
            return pos, recs, 7
        code, rec = record_at(plain, pos)
        if code:
            return pos, recs, code
        recs.append(rec)
        pos += 4 + rec[1]
    return pos, recs, SPAN_END


def plausible_offsets(plain):
    """Ascending offsets whose first record passes the candidate test's own checks (the rule, and refID, pos, next refID and
    next pos >= -1), found with numpy: what the candidate pass would walk on from."""
    n = len(plain)
    if n < 36:
        return []
    a = np.frombuffer(bytes(plain) + bytes(8), dtype=np.uint8).astype(np.int64)
    m = n - 35

    def le32(at):
        return a[at:at + m] | a[at + 1:at + 1 + m] << 8 | a[at + 2:at + 2 + m] << 16 | a[at + 3:at + 3 + m] << 24

    def signed(v):
        return np.where(v >= 1 << 31, v - (1 << 32), v)

    bs, lseq = signed(le32(0)), le32(20)
    lname, ncig = a[12:12 + m], a[16:16 + m] | a[17:17 + m] << 8
    ok = (bs >= 32) & (bs <= B.MAX_BLOCK_SIZE) & (np.arange(m) + 4 + bs <= n) & (lname != 0) & (lseq <= 0x7fffffff)
    ok &= 32 + lname + 4 * ncig + (lseq + 1) // 2 + lseq <= bs
    for at in (4, 8, 24, 28):
        ok &= signed(le32(at)) >= -1
    out = []
    for p in np.flatnonzero(ok).tolist():
        if plain[p + 36 + plain[p + 12] - 1] == 0:
            out.append(p)
    return out


class Model:
    """The index over one chunk: rows per span on demand (from the plausible offsets, computed once), then index()."""

    def __init__(self, plain):
        self.plain = bytes(plain)
        self.first_ok = plausible_offsets(self.plain)
        self._ok = set(self.first_ok)
        self._arr = np.asarray(self.first_ok, dtype=np.int64)

    def rows(self, k, S, K, start):
        """The first K candidates of span k: [(entry, exit, records, stop)], offsets absolute."""
        n, lo, hi = len(self.plain), k * S, (k + 1) * S
        tested = [start] if k == start // S else self._arr[np.searchsorted(self._arr, lo):np.searchsorted(self._arr, hi)].tolist()
        out = []
        for p in tested:
            if p not in self._ok or p + 36 > n:
                continue
            ex, recs, stop = span_walk(self.plain, p, hi)
            if 1 <= stop <= 4:
                continue
            out.append((p, ex, len(recs), stop))
            if len(out) == K:
                break
        return out

    def index(self, start, cap, S, K):
        """-> (records, next, error, error_off, stats) with stats = {entered, hits, settled, settled_spans}."""
        plain, n = self.plain, len(self.plain)
        table, pos, nxt, err, eoff = [], start, start, 0, 0
        st = {"entered": 0, "hits": 0, "settled": 0, "settled_spans": []}
        while len(table) < cap:
            nxt = pos
            if n - pos < 4:
                break
            k = pos // S
            st["entered"] += 1
            hit = [r for r in self.rows(k, S, K, start) if r[0] == pos]
            if hit:
                st["hits"] += 1
                _, ex, count, stop = hit[0]
            else:
                st["settled"] += 1
                st["settled_spans"].append(k)
                ex, recs, stop = span_walk(plain, pos, (k + 1) * S)
                count = len(recs)
            # the write pass: the span again from its verified entry, up to the table's room
            wex, wrecs, wstop = span_walk(plain, pos, (k + 1) * S, cap - len(table))
            table += wrecs
            if count > len(wrecs):
                assert wstop == 7
                nxt = wex
                break
            assert (wex, len(wrecs)) == (ex, count)
            nxt = pos = ex
            if len(table) == cap:
                break
            if 1 <= stop <= 4:
                err, eoff = stop, ex
                break
            if stop != SPAN_END:
                break
        return table, nxt, err, eoff, st


def model_index(plain, start, cap, S, K):
    return Model(plain).index(start, cap, S, K)


# ------------------------------------------------------------------------------------------------------------------ inputs
def short_read_stream(seed, n_records, l_seq=150):
    """Well-formed short-read records: random SEQ, qualities 2 .. 40, mapped positions, a CIGAR op, a few aux bytes."""
    gen = random.Random(seed)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_records):
        name = b"r%07d/%d\0" % (gen.randrange(10 ** 7), i % 2 + 1)
        body = struct.pack("<iiBBHHHIiii", gen.randrange(24), gen.randrange(1 << 27), len(name), gen.randrange(61), 4680, 1, gen.choice((0, 16, 99, 147)),
                           l_seq, gen.randrange(24), gen.randrange(1 << 27), gen.randrange(-500, 500))
        body += name + struct.pack("<I", l_seq << 4) + rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
        body += rng.integers(2, 41, l_seq, dtype=np.uint8).tobytes() + b"NMC" + bytes([gen.randrange(5)]) + b"ASC" + bytes([gen.randrange(150)])
        out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


def decoy_stream(S, n_decoys):
    """-> (stream, span of the decoys, the true entry of that span).  A record whose aux bytes are n_decoys whole valid
    records of 40 bytes that begin 2 bytes into span 3 and tile the aux bytes to the host record's end, so each decoy's chain
    is self-consistent and rejoins the true one at the record behind the host record, which starts later in span 3.  With K
    slots, n_decoys >= K leaves the true entry out of the rows (the span is settled by the serial rule); n_decoys < K keeps it."""
    assert n_decoys * 40 + 2 < S
    gen = random.Random(S * 16 + n_decoys)
    out = []
    B.records_until(gen, 0, 3 * S - 40, out)
    small = B.build_record(2, 0, 0, aux=2)
    assert len(small) == 40
    host = B.build_record(2, 0, 0, aux=b"\xff" * 4 + small * n_decoys)   # 38 bytes of header: the decoys begin at 3 * S + 2
    out.append(host)
    entry = 3 * S - 40 + len(host)
    assert entry == 3 * S + 2 + 40 * n_decoys
    B.records_until(gen, entry, entry + 2 * S + 77, out)
    return b"".join(out), 3, entry


def boundary_stream(S):
    """-> (stream, facts): records of 40-400 bytes with one that starts exactly on a span boundary, one longer than 100
    spans, a span in which no record starts (inside the long one), two records that start in one span, and an incomplete last record."""
    gen = random.Random(S)
    out = []
    B.records_until(gen, 0, 5 * S, out)
    on_boundary = 5 * S
    out.append(B.record_of_size(gen, 150))
    long_at = 5 * S + 150
    out.append(B.record_of_size(gen, 101 * S + 13))
    pos = long_at + 101 * S + 13
    out += [B.build_record(2, 0, 0, aux=2)] * 3                        # 40 bytes each: two of them start in one span
    pos += 120
    B.records_until(gen, pos, pos + 3 * S + 41, out)
    stream = b"".join(out)
    tail = B.record_of_size(gen, 120)[:57]
    return stream + tail, {"on_boundary": on_boundary, "long_at": long_at, "complete": len(stream)}


def case_file(path, cases):
    """cases [(plain, start, cap, S, K)] as tests/cpp/bam_index_host.cpp reads them: per case five little-endian u64
    (bytes, start, cap, S, K) and the bytes."""
    with open(path, "wb") as f:
        for plain, start, cap, S, K in cases:
            f.write(struct.pack("<5Q", len(plain), start, cap, S, K))
            f.write(plain)


def result_line(result):
    """A model result as the host program prints it."""
    table, nxt, err, eoff, st = result
    return "n %d next %d error %d at %d entered %d hits %d settled %d :%s" % (
        len(table), nxt, err, eoff, st["entered"], st["hits"], st["settled"], "".join(" %d,%d,%d,%d" % r for r in table))
