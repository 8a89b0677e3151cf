"""What tests/test_bam_chunk_reference_cpu.py and tests/test_gpu_bam_chunk.py share: plain-Python references of the three
stages behind the device inflate (record walk, SEQ decode, gather of passing records), builders of BAM records and BGZF
members with every field free, the seeded input generators, and thin ctypes wrappers over the ts_bam_chunk_* entry points.
No test functions live here.

The references restate the host route (bamSubset in include/teloscope_mi355x_io.hpp), not the kernels: ref_walk is its
record loop with its checks in its order, ref_decode is the table =ACMGRSVTWYHKDBN with the high nibble first."""
import ctypes as C
import random
import struct
import zlib

import numpy as np

SEQ_LETTERS = b"=ACMGRSVTWYHKDBN"
MAX_BLOCK_SIZE = 256 << 20
FUZZ_SEEDS = 600                    # streams of the walk fuzz: what the CPU file pins is what the GPU file walks
# byte offsets of the fields the walk reads, from the record's block_size field
AT_BLOCK_SIZE, AT_L_READ_NAME, AT_N_CIGAR_OP, AT_L_SEQ, AT_NAME = 0, 12, 16, 20, 36


# ------------------------------------------------------------------------------------------------------------ references
def ref_walk(plain, start, cap):
    """-> (records, next, error, error_off); a record is (off, block_size, seq_at, l_seq) as ts_bam_record holds it."""
    pos, recs, n = start, [], len(plain)
    while len(recs) < cap and n - pos >= 4:
        bs = struct.unpack_from("<i", plain, pos)[0]
        if bs < 32 or bs > MAX_BLOCK_SIZE:
            return recs, pos, 1, pos
        if n - pos < 4 + bs:
            break
        core = pos + 4
        lname, ncig = plain[core + 8], struct.unpack_from("<H", plain, core + 12)[0]
        lseq = struct.unpack_from("<I", plain, core + 16)[0]
        seq_at = 32 + lname + 4 * ncig
        if lname == 0 or lseq > 0x7fffffff:
            return recs, pos, 2, pos
        if seq_at + (lseq + 1) // 2 + lseq > bs:
            return recs, pos, 3, pos
        if plain[core + 32 + lname - 1] != 0:
            return recs, pos, 4, pos
        recs.append((pos, bs, 4 + seq_at, lseq))
        pos += 4 + bs
    return recs, pos, 0, 0


_HIGH = bytes(SEQ_LETTERS[b >> 4] for b in range(256))
_LOW = bytes(SEQ_LETTERS[b & 15] for b in range(256))


def ref_decode(plain, rec):
    """The l_seq bases of a record as ASCII: two per packed byte, the high nibble first."""
    off, _, seq_at, l_seq = rec
    packed = bytes(plain[off + seq_at:off + seq_at + (l_seq + 1) // 2])
    out = bytearray(2 * len(packed))
    out[0::2] = packed.translate(_HIGH)
    out[1::2] = packed.translate(_LOW)
    return bytes(out[:l_seq])


def ref_gather(plain, recs, pass_bytes):
    """-> (the passing records whole, block_size field included, in input order; how many they are)."""
    kept = [bytes(plain[r[0]:r[0] + 4 + r[1]]) for r, p in zip(recs, pass_bytes) if p]
    return b"".join(kept), len(kept)


# -------------------------------------------------------------------------------------------------------------- builders
def pattern_bytes(n, mul, add):
    """n non-zero bytes of a fixed pattern."""
    return ((np.arange(n, dtype=np.uint64) * mul + add) % 255 + 1).astype(np.uint8).tobytes()


def build_record(l_read_name=2, n_cigar_op=0, l_seq=0, seq=None, aux=0, name=None):
    """One BAM record, block_size field first.  name: l_read_name bytes (default: non-zero bytes and a NUL); seq: the raw
    packed SEQ, (l_seq + 1) // 2 bytes (default zeros); aux: a length or the bytes.  CIGAR and aux bytes are non-zero
    patterns that differ from each other, QUAL is 0xff."""
    if name is None:
        name = bytes(0x41 + i % 26 for i in range(l_read_name - 1)) + b"\0"
    if seq is None:
        seq = bytes((l_seq + 1) // 2)
    if isinstance(aux, int):
        aux = pattern_bytes(aux, 7, 3)
    assert len(name) == l_read_name and len(seq) == (l_seq + 1) // 2
    body = struct.pack("<iiBBHHHIiii", -1, -1, l_read_name, 0, 4680, n_cigar_op, 4, l_seq, -1, -1, 0)
    body += name + pattern_bytes(4 * n_cigar_op, 37, 0x90) + seq + b"\xff" * l_seq + aux
    return struct.pack("<i", len(body)) + body


def pack_bases(bases):
    """ASCII bases (letters of =ACMGRSVTWYHKDBN) as BAM packs them: two per byte, the first in the high nibble."""
    codes = [SEQ_LETTERS.index(c) for c in bases] + [0]
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(bases), 2))


def record_of_size(gen, total):
    """A valid record of exactly `total` bytes (>= 37), its spare room in aux."""
    lname, ncig, lseq = gen.choice((1, 2, 5, 8)), gen.randrange(3), gen.randrange(8)
    if 36 + lname + 4 * ncig + (lseq + 1) // 2 + lseq > total:
        lname, ncig, lseq = 1, 0, 0
    rec = build_record(lname, ncig, lseq, seq=bytes(gen.randrange(256) for _ in range((lseq + 1) // 2)),
                       aux=total - (36 + lname + 4 * ncig + (lseq + 1) // 2 + lseq))
    assert len(rec) == total
    return rec


def records_until(gen, pos, target, out):
    """Appends valid records to `out` so that the stream, now `pos` bytes long, becomes exactly `target` bytes long."""
    assert target == pos or target - pos >= 37
    while target - pos > 800:
        r = record_of_size(gen, gen.randrange(40, 400))
        out.append(r)
        pos += len(r)
    if target > pos:
        out.append(record_of_size(gen, target - pos))


WALK_WINDOW, WALK_SMALL_WINDOW, WALK_HEADER = 16384, 1024, 292


def staged_windows(plain, start=0):
    """A model of WHEN the device walk stages bytes, from its description alone: before a record at pos it needs the
    header region [pos, pos + 292) (or up to the stream's end where less is left) inside the staged window; when it is
    not, it stages a window from pos rounded down to 16 bytes, 16 KB long, or 1 KB when the record before had a
    block_size above 8 192.  -> [(pos that forced it, window start, window bytes)]"""
    out, wlo, whi, last, n = [], 0, 0, 0, len(plain)
    for pos, bs, _, _ in ref_walk(plain, start, 1 << 30)[0]:
        want = n if n - pos < WALK_HEADER else pos + WALK_HEADER
        if pos < wlo or want > whi:
            size = WALK_SMALL_WINDOW if last > WALK_WINDOW // 2 else WALK_WINDOW
            wlo = pos & ~15
            whi = wlo + size
            out.append((pos, wlo, size))
        last = bs
    return out


def placement_stream(seed, first_block_size, d):
    """-> (stream, offset of the placed record): a record with a 255-byte name (the walk's longest header region: its
    name's NUL is byte 290 of the record) starts d bytes before the end of a window the walk has staged.  With
    first_block_size == 0 that is the first window, [0, 16384).  Otherwise a record of that block_size starts at 12 000,
    inside the first window, and ends beyond it, so the record behind it forces the next window: 16 KB for a block_size
    up to 8 192, 1 KB above; the placed record lies d bytes before THAT window's end.  No record before the placed one
    starts within 292 bytes of the window's end (that would stage a new window early)."""
    gen = random.Random(seed)
    out, pos, whi = [], 0, WALK_WINDOW
    if first_block_size:
        records_until(gen, 0, 12000, out)
        out.append(record_of_size(gen, 4 + first_block_size))
        pos = 12000 + 4 + first_block_size
        assert pos + WALK_HEADER > WALK_WINDOW
        whi = (pos & ~15) + (WALK_SMALL_WINDOW if first_block_size > WALK_WINDOW // 2 else WALK_WINDOW)
    records_until(gen, pos, whi - d, out)
    lseq, ncig = gen.randrange(600), gen.randrange(4)
    out.append(build_record(255, ncig, lseq, seq=bytes(gen.randrange(256) for _ in range((lseq + 1) // 2)), aux=gen.randrange(50)))
    pos = whi - d + len(out[-1])
    records_until(gen, pos, pos + (18000 if first_block_size else 2000) + gen.randrange(300), out)
    return b"".join(out), whi - d


def verdict_cases():
    """Hand-written streams and what the walk must say about them, written out:
    [(name, stream, cap, (records, next, error, error_off))]."""
    ok = build_record(2, 0, 4, seq=b"\x12\x48")                     # 44 bytes: block_size 40, SEQ at 38
    assert len(ok) == 44
    first, second = (0, 40, 38, 4), (44, 40, 38, 4)

    def patched(at, fmt, value, rec=ok):
        m = bytearray(rec)
        struct.pack_into(fmt, m, at, value)
        return bytes(m)

    return [
        ("two records that fit exactly, no aux", ok + ok, 8, ([first, second], 88, 0, 0)),
        ("l_read_name 0 and fields that exceed: lengths first",
         ok + patched(AT_L_SEQ, "<I", 100, patched(AT_L_READ_NAME, "<B", 0)), 8, ([first], 44, 2, 44)),
        ("l_seq 0x80000000", ok + patched(AT_L_SEQ, "<I", 0x80000000), 8, ([first], 44, 2, 44)),
        ("bad block_size on a record that does not fit either: block_size first", ok + struct.pack("<i", 31) + bytes(10), 8,
         ([first], 44, 1, 44)),
        ("valid block_size, incomplete, l_read_name 0: stop, no error", ok + patched(AT_L_READ_NAME, "<B", 0)[:43], 8,
         ([first], 44, 0, 0)),
        ("fields exceed by exactly one byte", ok + patched(AT_BLOCK_SIZE, "<i", 39)[:43], 8, ([first], 44, 3, 44)),
        ("fields exceed and the name is not terminated: fields first",
         patched(AT_NAME + 1, "<B", 7, patched(AT_BLOCK_SIZE, "<i", 39)[:43]), 8, ([], 0, 3, 0)),
        ("name not NUL-terminated", ok + patched(AT_NAME + 1, "<B", 7), 8, ([first], 44, 4, 44)),
        ("block_size 256 MiB in a 40-byte stream: incomplete", struct.pack("<i", MAX_BLOCK_SIZE) + bytes(36), 8, ([], 0, 0, 0)),
        ("block_size 256 MiB + 1", struct.pack("<i", MAX_BLOCK_SIZE + 1) + bytes(36), 8, ([], 0, 1, 0)),
        ("block_size 31", ok + patched(AT_BLOCK_SIZE, "<i", 31), 8, ([first], 44, 1, 44)),
        ("block_size 0", patched(AT_BLOCK_SIZE, "<i", 0), 8, ([], 0, 1, 0)),
        ("block_size -1", ok + ok + patched(AT_BLOCK_SIZE, "<i", -1), 8, ([first, second], 88, 1, 88)),
        ("block_size INT32_MIN", patched(AT_BLOCK_SIZE, "<i", -2 ** 31), 8, ([], 0, 1, 0)),
        ("table full before the bad record", ok + patched(AT_BLOCK_SIZE, "<i", 0), 1, ([first], 44, 0, 0)),
        ("three bytes left", ok + b"\x28\x00\x00", 8, ([first], 44, 0, 0)),
    ]


def fuzz_stream(seed):
    """-> (stream, record boundaries inside it, kind): 1-59 valid records, then ONE targeted mutation chosen by seed % 6:
    none, block_size, lengths, l_seq := block_size, the name's terminator, a truncated tail."""
    gen = random.Random(seed)
    recs = []
    for _ in range(gen.randrange(1, 60)):
        lname = gen.choice((1, 2, 255, gen.randrange(1, 256)))
        ncig = gen.choice((0, 1, gen.randrange(40)))
        lseq = gen.choice((0, 1, 2, gen.randrange(5000)))
        name = bytes(gen.randrange(1, 256) for _ in range(lname - 1)) + b"\0"
        seq = bytes(gen.getrandbits(8) for _ in range((lseq + 1) // 2))
        recs.append(build_record(lname, ncig, lseq, seq=seq, aux=gen.randrange(200), name=name))
    starts = [0]
    for r in recs:
        starts.append(starts[-1] + len(r))
    m = bytearray(b"".join(recs))
    kind = seed % 6
    at = starts[gen.randrange(len(recs))]
    if kind == 1:
        struct.pack_into("<i", m, at, gen.choice((-1, 0, 31, MAX_BLOCK_SIZE + 1, -2 ** 31)))
    elif kind == 2:
        if gen.randrange(2):
            m[at + AT_L_READ_NAME] = 0
        else:
            struct.pack_into("<I", m, at + AT_L_SEQ, gen.choice((0x80000000, 0xffffffff)))
    elif kind == 3:
        struct.pack_into("<I", m, at + AT_L_SEQ, struct.unpack_from("<i", m, at)[0])
    elif kind == 4:
        m[at + AT_NAME + m[at + AT_L_READ_NAME] - 1] = gen.randrange(1, 256)
    elif kind == 5:
        del m[len(m) - gen.randrange(300):]
    return bytes(m), [s for s in starts if s <= len(m)], kind


def carry_plan(seed):
    """-> (stream, fills): a stream of several MiB (short records, one of ~1.5 MiB, one of ~200 KB) and how it is fed to a
    chunk: per fill the members' uncompressed sizes (0 .. 65 536, empty members included) and the walk's table size.  Some
    fills end exactly at a record's end (nothing to carry), some walks take only three records (a long tail to carry)."""
    gen = random.Random(seed)
    rng = np.random.default_rng(seed)
    codes = np.frombuffer(b"\x11\x12\x14\x18\x21\x22\x24\x28\x41\x42\x44\x48\x81\x82\x84\x88", dtype=np.uint8)
    recs, ends, total = [], [], 0
    while total < (4 << 20):
        i = len(recs)
        lseq = 1_000_001 if i == 700 else 131_073 if i == 1500 else gen.choice((0, 1, gen.randrange(200), gen.randrange(4000)))
        r = build_record(gen.choice((1, 2, 30, 255)), gen.randrange(3), lseq, seq=rng.choice(codes, (lseq + 1) // 2).tobytes(),
                         aux=gen.randrange(60))
        recs.append(r)
        total += len(r)
        ends.append(total)
    assert len(recs) > 1500
    stream = b"".join(recs)
    fills, fed = [], 0
    while fed < len(stream):
        sizes = []
        for _ in range(gen.randrange(1, 9)):
            s = gen.choice((0, 65536, gen.randrange(1, 300), gen.randrange(1, 65537), gen.randrange(1, 65537)))
            sizes.append(min(s, len(stream) - fed - sum(sizes)))
        if len(fills) % 7 == 6:                                     # end this fill at a record's end where one is near
            before = fed + sum(sizes[:-1])
            k = int(np.searchsorted(ends, before + 1))
            if k < len(ends) and ends[k] - before <= 65536:
                sizes[-1] = ends[k] - before
        fed += sum(sizes)
        fills.append((sizes, 3 if len(fills) % 5 == 3 else 1 << 16))
    return stream, fills


def carry_move(size, carry_from):
    """Which device-to-device move ts_bam_chunk_inflate needs for the tail [carry_from, size)."""
    carry = size - carry_from
    if carry == 0:
        return "none"
    if carry_from == 0:
        return "in place"
    return "direct" if carry_from >= carry else "through the temporary"


def simulate_carry(stream, fills):
    """The moves the plan causes when the walk answers as ref_walk does: [(move, chunk size after the fill)]."""
    chunk, fed, carry_from, out = b"", 0, 0, []
    for sizes, cap in fills:
        move = carry_move(len(chunk), carry_from)
        n = sum(sizes)
        chunk = chunk[carry_from:] + stream[fed:fed + n]
        fed += n
        out.append((move, len(chunk)))
        carry_from = ref_walk(chunk, 0, cap)[1]
    return out


def pack_members(plain, sizes, mode="mixed"):
    """plain cut into BGZF members of the given uncompressed sizes -> (compressed bytes, [(src_off, payload_len, isize, crc,
    dst_off)]) with dst_off counted from the first member's output.  Payloads are stored deflate blocks or zlib level 1
    (mode "stored", "zlib" or "mixed": alternating where both fit the 65 536 bytes a payload may have)."""
    assert sum(sizes) == len(plain)
    comp, descs, at = bytearray(), [], 0
    for i, isize in enumerate(sizes):
        piece = bytes(plain[at:at + isize])
        stored = b"\x01" + struct.pack("<HH", isize, isize ^ 0xffff) + piece if isize <= 65531 else None
        if stored is not None and (mode == "stored" or (mode == "mixed" and i % 2 == 0)):
            payload = stored
        else:
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            payload = co.compress(piece) + co.flush()
            if len(payload) > 65536 and stored is not None:
                payload = stored
        assert len(payload) <= 65536, "a member of %d bytes does not fit a BGZF payload" % isize
        descs.append((len(comp), len(payload), isize, zlib.crc32(piece) & 0xFFFFFFFF, at))
        comp += payload
        at += isize
    return bytes(comp), descs


def members_of(plain, member=65280, mode="stored"):
    return pack_members(plain, [min(member, len(plain) - a) for a in range(0, len(plain), member)], mode)


# -------------------------------------------------------------------------------------------- the library through ctypes
def hip():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        return lib
    raise RuntimeError("libamdhip64 is not loadable")


def device_bytes(ptr, n):
    """n bytes of device memory, once the device is idle."""
    h = hip()
    assert h.hipDeviceSynchronize() == 0
    buf = C.create_string_buffer(max(n, 1))
    if n:
        assert h.hipMemcpy(buf, C.c_void_p(ptr), n, 2) == 0
    return buf.raw[:n]


def to_device(ptr, data):
    assert hip().hipMemcpy(C.c_void_p(ptr), bytes(data), len(data), 1) == 0


def table_of(records):
    """Records (off, block_size, seq_at, l_seq) as a ts_bam_record array."""
    from teloscope_amd import _capi as K
    arr = (K.BamRecord * max(1, len(records)))()
    for i, (off, bs, seq_at, lseq) in enumerate(records):
        arr[i].off, arr[i].block_size, arr[i].seq_at, arr[i].l_seq = off, bs, seq_at, lseq
    return arr


class Chunk:
    """A ts_bam_chunk and a host copy of what it must hold."""

    def __init__(self, ctx, compressed_cap, plain_cap):
        from teloscope_amd import _capi as K
        self.K, self.L, self.ctx = K, K.lib(), ctx
        self.ptr = self.L.ts_bam_chunk_create(ctx, compressed_cap, plain_cap)
        assert self.ptr, self.L.ts_last_error(ctx)
        self.mirror = b""

    def close(self):
        if self.ptr:
            self.L.ts_bam_chunk_destroy(self.ptr)
            self.ptr = None

    def size(self):
        return int(self.L.ts_bam_chunk_size(self.ptr))

    def read(self, off, n):
        buf = C.create_string_buffer(max(n, 1))
        assert self.L.ts_bam_chunk_read(self.ptr, off, n, buf) == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        return buf.raw[:n]

    def inflate(self, compressed, descs, carry_from, stream=None):
        """The bare call: descs as pack_members gives them, dst_off counted from the chunk's first byte."""
        blocks = (self.K.BgzfBlock * max(1, len(descs)))()
        for i, (src, plen, isize, crc, dst) in enumerate(descs):
            blocks[i].src_off, blocks[i].payload_len, blocks[i].isize, blocks[i].crc, blocks[i].dst_off = src, plen, isize, crc, dst
        return self.L.ts_bam_chunk_inflate(self.ptr, compressed, len(compressed), blocks, len(descs), carry_from, stream)

    def fill(self, plain, members, carry_from=None):
        """The chunk's next contents: its tail from carry_from (default: nothing is carried), then `plain`, which `members`
        (pack_members) holds.  Inflate + status must be OK and the chunk must read back as exactly those bytes."""
        K = self.K
        carry_from = len(self.mirror) if carry_from is None else carry_from
        carry = len(self.mirror) - carry_from
        compressed, descs = members
        rc = self.inflate(compressed, [(s, p, n, c, d + carry) for s, p, n, c, d in descs], carry_from)
        assert rc == K.TS_OK, self.L.ts_last_error(self.ctx)
        st = K.BgzfStatus()
        assert self.L.ts_bam_chunk_status(self.ptr, C.byref(st)) == K.TS_OK
        assert (st.code, st.block) == (K.BGZF_OK, len(descs)), (st.code, st.block)
        self.mirror = self.mirror[carry_from:] + bytes(plain)
        assert self.size() == len(self.mirror)
        got = self.read(0, len(self.mirror))
        assert got == self.mirror, "the chunk differs from the bytes intended, first at byte %d" % next(
            i for i, (a, b) in enumerate(zip(got, self.mirror)) if a != b)
        return self.mirror

    def fill_plain(self, plain, carry_from=None, member=65280, mode="stored"):
        return self.fill(plain, members_of(plain, member, mode), carry_from)

    def walk(self, start, cap):
        """-> (records as tuples, next, error, error_off).  The table handed over has one entry more than cap; what lies
        behind the records taken must be as it was."""
        K = self.K
        arr = (K.BamRecord * (cap + 1))()
        C.memset(arr, 0xEE, C.sizeof(arr))
        n, nxt, err, eoff = C.c_uint64(7), C.c_uint64(7), C.c_int(7), C.c_uint64(7)
        rc = self.L.ts_bam_chunk_walk(self.ptr, start, arr, cap, C.byref(n), C.byref(nxt), C.byref(err), C.byref(eoff))
        assert rc == K.TS_OK, self.L.ts_last_error(self.ctx)
        assert n.value <= cap
        recs = []
        for i in range(n.value):
            assert arr[i].reserved == 0
            recs.append((arr[i].off, arr[i].block_size, arr[i].seq_at, arr[i].l_seq))
        rest = bytes(arr)[n.value * C.sizeof(K.BamRecord):]
        assert rest == b"\xee" * len(rest), "the walk wrote behind the records it reported"
        return recs, nxt.value, err.value, eoff.value

    def decode(self, records, batch, stream=None):
        return self.L.ts_bam_chunk_decode(self.ptr, table_of(records), len(records), batch, stream)

    def gather(self, records, d_pass, cap, stream=None, fill=0xA5):
        """-> (rc, host_out as the call left it: cap bytes prefilled with `fill`, *bytes, *n_passed)"""
        out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
        nbytes, npassed = C.c_uint64(0xdead), C.c_uint64(0xdead)
        rc = self.L.ts_bam_chunk_gather(self.ptr, table_of(records), len(records), d_pass, out, cap, C.byref(nbytes),
                                        C.byref(npassed), stream)
        return rc, (out.raw if cap else b""), nbytes.value, npassed.value


class ReadBatch:
    """A batch of segments of the given lengths (tips-only unless tips=0), normally on a read-filter context."""

    def __init__(self, ctx, lens, tips=1, capacity=1 << 16):
        from teloscope_amd import _capi as K
        self.K, self.L, self.ctx, self.lens = K, K.lib(), ctx, list(lens)
        n = len(self.lens)
        self.ptr = self.L.ts_batch_create(ctx, (C.c_uint64 * max(1, n))(*self.lens), None, n, tips, capacity)
        assert self.ptr, self.L.ts_last_error(ctx)
        info = K.BatchInfo()
        assert self.L.ts_batch_get_info(self.ptr, C.byref(info)) == K.TS_OK
        self.input_bytes = int(info.input_bytes)
        self.offsets = [int(self.L.ts_batch_segment_offset(self.ptr, i)) for i in range(n)]

    def close(self):
        if self.ptr:
            self.L.ts_batch_destroy(self.ptr)
            self.ptr = None

    def image(self):
        """The whole input buffer, input_bytes of it, from the device."""
        p = self.L.ts_batch_input_ptr(self.ptr)
        assert p
        return device_bytes(p, self.input_bytes)

    def expected_image(self, reads):
        """Segment i holds reads[i]; every byte between and behind the segments is zero."""
        img = bytearray(self.input_bytes)
        for off, ln, r in zip(self.offsets, self.lens, reads):
            assert len(r) == ln and off + ln <= self.input_bytes
            img[off:off + ln] = r
        return bytes(img)
