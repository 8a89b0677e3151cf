"""The three stages behind the device inflate of --bam-subset, one by one against the plain references of tests/bamchunk.py
(pinned without a device by tests/test_bam_chunk_reference_cpu.py): the record walk's table, next, error and error_off; the
decoded bases, byte for byte, with the zeros between and behind them; what a chunk holds after a fill with a carried tail;
the gathered records with *bytes and *n_passed.  Equality is exact everywhere.  One context and one chunk serve the whole
module, reused across cases on purpose; every fill asserts that the chunk reads back as the bytes intended.
tests/test_gpu_bam_device.py checks the route as a whole against the host route."""
import ctypes as C
import random
import types

import numpy as np
import pytest

from tests import bamchunk as B
from tests import harness as H
from tests import seqgen
from tests.backends import OracleReadFilter

pytestmark = pytest.mark.gpu
CHUNK_BYTES = 8 << 20


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("--fastq-subset -l 42")
    rf = ta.ReadTelomereFilter(user_input(opts, device=0))
    chunk = B.Chunk(rf._ctx.ptr, CHUNK_BYTES, CHUNK_BYTES)
    yield types.SimpleNamespace(K=K, L=K.lib(), ta=ta, opts=opts, user_input=user_input, rf=rf, ctx=rf._ctx.ptr, chunk=chunk)
    chunk.close()
    rf.close()


def check_walk(chunk, plain, start, cap, what=""):
    got, exp = chunk.walk(start, cap), B.ref_walk(plain, start, cap)
    assert got[1:] == exp[1:], "%s: (next, error, error_off) %r, reference %r" % (what, got[1:], exp[1:])
    assert len(got[0]) == len(exp[0]), "%s: %d records, reference %d" % (what, len(got[0]), len(exp[0]))
    for i, (g, e) in enumerate(zip(got[0], exp[0])):
        assert g == e, "%s: record %d is %r, reference %r" % (what, i, g, e)
    return got


def assert_same_bytes(got, exp, what):
    assert len(got) == len(exp), "%s: %d bytes, expected %d" % (what, len(got), len(exp))
    if got != exp:
        at = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
        raise AssertionError("%s: first difference at byte %d: %r, expected %r" % (what, at, got[at:at + 16], exp[at:at + 16]))


# ================================================================================================================== decode
DECODE_LENGTHS = list(range(1, 41)) + list(range(1008, 1041)) + list(range(2032, 2065)) + [4095, 4096, 4097, 70001]


def decode_stream(seed):
    """16 reads of 32 bases in which, between them, every code stands at every byte lane of a 16-byte store (base i of read
    k has code (i + k + seed) % 16: even lanes come from high nibbles, odd ones from low nibbles), then reads of
    DECODE_LENGTHS with random packed bytes, with name lengths and CIGAR counts that move SEQ through every alignment, and
    a record without SEQ among them."""
    gen = random.Random(seed)
    recs = []
    for k in range(16):
        codes = [(i + k + seed) % 16 for i in range(32)]
        recs.append(B.build_record(1 + k % 8, k % 3, 32, seq=bytes(codes[i] << 4 | codes[i + 1] for i in range(0, 32, 2)), aux=k))
    for j, n in enumerate(DECODE_LENGTHS):
        if j == 50:
            recs.append(B.build_record(3, 1, 0, aux=9))
        seq = bytes(gen.getrandbits(8) for _ in range((n + 1) // 2))
        recs.append(B.build_record(1 + (j * 5 + seed) % 11, (j + seed) % 4, n, seq=seq, aux=(j * 3) % 17))
    return b"".join(recs)


def decoded_batch(env, seed, batch=None):
    chunk = env.chunk
    plain = chunk.fill_plain(decode_stream(seed))
    recs, nxt, err, _ = check_walk(chunk, plain, 0, 1000, "decode stream %d" % seed)
    assert (nxt, err) == (len(plain), 0) and len(recs) == 16 + len(DECODE_LENGTHS) + 1
    with_seq = [r for r in recs if r[3]]
    assert [r[3] for r in with_seq] == [32] * 16 + DECODE_LENGTHS
    assert {(r[0] + r[2]) % 8 for r in with_seq} == set(range(8))                  # every source alignment
    reads = [B.ref_decode(plain, r) for r in with_seq]
    assert {(i % 16, c) for r in reads[:16] for i, c in enumerate(r)} == {(i, c) for i in range(16) for c in B.SEQ_LETTERS}
    if batch is None:
        batch = B.ReadBatch(env.ctx, [r[3] for r in with_seq])
    assert chunk.decode(with_seq, batch.ptr) == env.K.TS_OK, env.L.ts_last_error(env.ctx)
    assert all(o % 16 == 0 for o in batch.offsets)
    assert_same_bytes(batch.image(), batch.expected_image(reads), "input buffer after decoding stream %d" % seed)
    return batch


def test_decode_every_code_lane_length_and_alignment(env):
    """The batch's whole input buffer against ref_decode: every segment's bases, zeros everywhere else; then other contents
    of the same lengths into the same batch, whose image must not depend on the first."""
    batch = decoded_batch(env, 1)
    try:
        decoded_batch(env, 2, batch)
        decoded_batch(env, 1, batch)
    finally:
        batch.close()


def telomeric_reads():
    rng = np.random.default_rng(5)
    reads = []
    for i in range(120):
        n = int(rng.integers(50, 6000))
        s = bytearray(seqgen.random_dna(rng, n).tobytes())
        if i % 3 == 0:
            t = ((b"TTAGGG" if i % 2 else b"CCCTAA") * 60)[:n]
            if i % 4 < 2:
                s[:len(t)] = t
            else:
                s[n - len(t):] = t
        if i % 10 == 7:
            s[n // 2] = ord("N")
        reads.append(bytes(s))
    return reads


def test_decode_scan_and_predicate_on_a_side_stream(env):
    """ts_bam_chunk_decode is asynchronous on `stream`: the same decode, scan and predicate on the null stream and on a
    stream of its own, each into a fresh batch, give the same input image and the pass bytes of the oracle's read filter.
    A fresh batch's input buffer is allocated and zeroed inside the decode call, on the null stream, which a non-blocking
    stream does not wait for: ts_bam_chunk_decode waits for that zeroing itself before it launches on `stream`."""
    import torch
    K, L, chunk = env.K, env.L, env.chunk
    reads = telomeric_reads()
    n = len(reads)
    plain = chunk.fill_plain(b"".join(B.build_record(1 + i % 9, i % 4, len(r), seq=B.pack_bases(r), aux=i % 13)
                                      for i, r in enumerate(reads)))
    recs = check_walk(chunk, plain, 0, 1000, "telomeric reads")[0]
    assert [B.ref_decode(plain, r) for r in recs] == reads
    exp = OracleReadFilter(env.opts).filter(reads)
    assert 10 < sum(exp) < n - 10
    dev = torch.device("cuda", 0)
    got = {}
    for name in ("null", "side"):
        stream = torch.cuda.Stream(device=dev) if name == "side" else None
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else None
        batch = B.ReadBatch(env.ctx, [len(r) for r in reads])
        try:
            d_pass = torch.full((n + 16,), 7, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            assert chunk.decode(recs, batch.ptr, sptr) == K.TS_OK, L.ts_last_error(env.ctx)
            assert L.ts_batch_scan(batch.ptr, None, sptr) == K.TS_OK, L.ts_last_error(env.ctx)
            assert L.ts_batch_read_pass(batch.ptr, C.c_void_p(d_pass.data_ptr()), sptr) == K.TS_OK
            flag = C.c_int(7)
            assert L.ts_batch_read_pass_status(batch.ptr, C.byref(flag)) == K.TS_OK and flag.value == 0
            if stream is not None:
                stream.synchronize()
            got[name] = d_pass.cpu().numpy().tolist()
            assert_same_bytes(batch.image(), batch.expected_image(reads), "input buffer, %s stream" % name)
        finally:
            batch.close()
    for name in ("null", "side"):
        assert got[name][n:] == [7] * 16, name
        assert [bool(x) for x in got[name][:n]] == exp, name
    assert got["side"] == got["null"]


def test_decode_refuses_what_does_not_fit(env):
    """TS_ERR_INVALID_ARG from the host, and nothing launched: the batch a refused call named keeps its image."""
    K, chunk = env.K, env.chunk
    INV = K.TS_ERR_INVALID_ARG
    plain = chunk.fill_plain(B.build_record(3, 1, 10, seq=b"\x12\x48\x12\x48\x12") + B.build_record(2, 0, 0, aux=4) +
                             B.build_record(5, 2, 7, seq=b"\x84\x21\x84\x20", aux=6))
    recs = check_walk(chunk, plain, 0, 10, "three records")[0]
    assert [r[3] for r in recs] == [10, 0, 7]
    good = [recs[0], recs[2]]
    other = env.ta.ReadTelomereFilter(env.user_input(env.opts, device=0))
    batches = [B.ReadBatch(env.ctx, [10, 7]), B.ReadBatch(env.ctx, [10, 0, 7]), B.ReadBatch(env.ctx, [10, 8]),
               B.ReadBatch(env.ctx, [10, 7], tips=0), B.ReadBatch(other._ctx.ptr, [10, 7]), B.ReadBatch(env.ctx, [10])]
    batch, with_empty, wrong_len, full_scan, foreign, too_few = batches
    try:
        assert chunk.decode(good, batch.ptr) == K.TS_OK
        image = batch.image()
        assert image == batch.expected_image([b"ACGTACGTAC", b"TGCATGC"])
        assert chunk.decode(recs, with_empty.ptr) == INV                           # a record with l_seq == 0
        assert chunk.decode(good, wrong_len.ptr) == INV                            # segment length != l_seq
        assert chunk.decode(good, full_scan.ptr) == INV                            # not a tips-only batch
        assert chunk.decode(good, foreign.ptr) == INV                              # a batch of another context
        assert chunk.decode(good, too_few.ptr) == INV                              # one segment per record
        off, bs, seq_at, lseq = recs[2]
        for bad in ((chunk.size() + 1, bs, seq_at, lseq),                          # off beyond the chunk
                    (off + 1, bs, seq_at, lseq),                                   # the record ends beyond the chunk
                    (off, bs, 4 + bs - 3, lseq),                                   # SEQ ends one byte beyond the record
                    (off, 31, seq_at, lseq),                                       # block_size the walk would refuse
                    (off, bs, seq_at, 0x80000000)):
            assert chunk.decode([recs[0], bad], batch.ptr) == INV, bad
        assert chunk.decode(good, None) == INV
        assert batch.image() == image
        for b in (with_empty, wrong_len, too_few):
            assert b.image() == bytes(b.input_bytes)
        assert chunk.decode(good, batch.ptr) == K.TS_OK and batch.image() == image
    finally:
        for b in batches:
            b.close()
        other.close()


# ==================================================================================================================== walk
@pytest.mark.parametrize("first_block_size", [0, 8192, 8193, 40000])
def test_walk_window_placement(env, first_block_size):
    """A record with the longest header region at every distance 0..300 from the end of the window the walk has staged when
    it gets there: the first 16 KB window; or the window forced behind a record that starts in the first window and ends
    beyond it, 16 KB for a block_size of 8 192, 1 KB for 8 193 and 40 000 (and from there back to 16 KB).  That the streams
    do this is asserted by tests/test_bam_chunk_reference_cpu.py against a model of the staging rule."""
    for d in range(301):
        plain = env.chunk.fill_plain(B.placement_stream(1000 * d + first_block_size, first_block_size, d)[0])
        recs, nxt, err, _ = check_walk(env.chunk, plain, 0, 1 << 10, "first block_size %d, d %d" % (first_block_size, d))
        assert (nxt, err) == (len(plain), 0) and len(recs) > 10


def test_walk_field_extremes_and_their_seq(env):
    """l_read_name 1, 2, 254, 255; n_cigar_op 0, 1, 65 535; l_seq 0, 1, 2, odd, even; aux none and large: the table, and
    the bases decoded from where the table says SEQ is."""
    gen = random.Random(3)
    recs = []
    for lname in (1, 2, 254, 255):
        for ncig in (0, 1, 65535):
            for lseq in (0, 1, 2) if ncig == 65535 else (0, 1, 2, 7, 8, 4001, 4000):
                seq = bytes(gen.getrandbits(8) for _ in range((lseq + 1) // 2))
                recs.append(B.build_record(lname, ncig, lseq, seq=seq, aux=70000 if (lname + lseq) % 5 == 0 else 0))
    plain = env.chunk.fill_plain(b"".join(recs))
    table, nxt, err, _ = check_walk(env.chunk, plain, 0, 1000, "field extremes")
    assert (len(table), nxt, err) == (len(recs), len(plain), 0)
    assert max(t[2] for t in table) == 36 + 255 + 4 * 65535
    with_seq = [t for t in table if t[3]]
    batch = B.ReadBatch(env.ctx, [t[3] for t in with_seq])
    try:
        assert env.chunk.decode(with_seq, batch.ptr) == env.K.TS_OK
        assert_same_bytes(batch.image(), batch.expected_image([B.ref_decode(plain, t) for t in with_seq]), "field extremes")
    finally:
        batch.close()


def test_walk_tails(env):
    gen = random.Random(11)
    body = b"".join(B.record_of_size(gen, gen.randrange(37, 600)) for _ in range(30)) + B.record_of_size(gen, 120)
    nxt_rec = B.build_record(255, 2, 40, aux=30)
    for extra in (0, 1, 2, 3, 4, 35, 36, 37, 291, 292, len(nxt_rec) - 1, len(nxt_rec)):
        plain = env.chunk.fill_plain(body + nxt_rec[:extra])
        recs, nxt, err, _ = check_walk(env.chunk, plain, 0, 1000, "tail of %d bytes" % extra)
        assert (len(recs), nxt, err) == ((32, len(plain), 0) if extra == len(nxt_rec) else (31, len(body), 0))
    for stream, n in ((b"", 0), (b"\x25\x00\x00", 0), (B.record_of_size(gen, 37), 1), (B.record_of_size(gen, 37)[:36], 0)):
        plain = env.chunk.fill_plain(stream)
        assert len(check_walk(env.chunk, plain, 0, 5, "stream of %d bytes" % len(stream))[0]) == n


def test_walk_table_sizes_and_starts(env):
    gen = random.Random(12)
    plain = env.chunk.fill_plain(b"".join(B.record_of_size(gen, gen.randrange(37, 900)) for _ in range(100)))
    table = B.ref_walk(plain, 0, 1000)[0]
    assert len(table) == 100
    for cap in (0, 99, 100, 101):
        recs, nxt, err, _ = check_walk(env.chunk, plain, 0, cap, "cap %d" % cap)
        assert (len(recs), nxt, err) == (min(cap, 100), len(plain) if cap >= 100 else table[cap][0], 0)
    for k, start in enumerate([t[0] for t in table] + [len(plain)]):
        assert len(check_walk(env.chunk, plain, start, 1000, "from record %d" % k)[0]) == 100 - k
        check_walk(env.chunk, plain, start, 2, "from record %d, two entries" % k)
    n = C.c_uint64(0)
    e = C.c_int(0)
    arr = (env.K.BamRecord * 4)()
    assert env.L.ts_bam_chunk_walk(env.chunk.ptr, len(plain) + 1, arr, 4, C.byref(n), C.byref(n), C.byref(e), C.byref(n)) == \
        env.K.TS_ERR_INVALID_ARG


@pytest.mark.parametrize("case", B.verdict_cases(), ids=lambda c: c[0])
def test_walk_verdicts(env, case):
    """The hand-written streams of the reference's own test, with the same literals."""
    _, stream, cap, expected = case
    env.chunk.fill_plain(stream)
    assert env.chunk.walk(0, cap) == expected


def test_walk_ignores_stale_bytes_behind_the_chunk(env):
    """After a long stream, a prefix of it that ends inside a record: the rest of that record is still in device memory
    behind the chunk's end, and the walk must stop at it all the same."""
    gen = random.Random(13)
    stream = b"".join(B.record_of_size(gen, gen.randrange(37, 700)) for _ in range(200))
    table = B.ref_walk(stream, 0, 1000)[0]
    for k, into in ((150, 50), (150, 3), (151, 4), (17, 36), (199, table[199][1] + 3), (60, 1), (0, 20)):
        env.chunk.fill_plain(stream)
        plain = env.chunk.fill_plain(stream[:table[k][0] + into])
        recs, nxt, err, _ = check_walk(env.chunk, plain, 0, 1000, "prefix ending %d bytes into record %d" % (into, k))
        assert (len(recs), nxt, err) == (k, table[k][0], 0)


def test_walk_fuzz(env):
    """The seeded streams whose distribution tests/test_bam_chunk_reference_cpu.py pins, each walked from a random record
    boundary with a random table size."""
    for seed in range(B.FUZZ_SEEDS):
        stream, starts, kind = B.fuzz_stream(seed)
        gen = random.Random(seed + 1_000_003)
        start, cap = gen.choice(starts), gen.choice((0, 1, 2, gen.randrange(1, 70), 1000))
        try:
            plain = env.chunk.fill_plain(stream)
            check_walk(env.chunk, plain, start, cap, "seed %d (kind %d) from %d, cap %d" % (seed, kind, start, cap))
        except AssertionError:
            print("walk fuzz: seed %d, kind %d, start %d, cap %d" % (seed, kind, start, cap))
            raise


# =================================================================================================================== carry
def test_carry_through_a_long_stream(env):
    """A stream of several MiB in members of random sizes, a few per fill, with carry_from = next of the walk before: the
    chunk's bytes after every fill, the concatenated tables against one walk of the whole stream, and all four ways a
    tail can move."""
    K, chunk = env.K, env.chunk
    stream, fills = B.carry_plan(7)
    whole = B.ref_walk(stream, 0, 1 << 30)
    assert whole[1:] == (len(stream), 0, 0)
    carry_from = chunk.size()                                        # what the chunk holds from the test before is dropped
    base, fed, table, moves = -carry_from, 0, [], []
    for sizes, cap in fills:
        moves.append(B.carry_move(chunk.size(), carry_from))
        piece = stream[fed:fed + sum(sizes)]
        fed += len(piece)
        base += carry_from
        mirror = chunk.fill(piece, B.pack_members(piece, sizes), carry_from)
        assert mirror == stream[base:fed]
        recs, carry_from, err, _ = check_walk(chunk, mirror, 0, cap, "fill %d" % len(moves))
        assert err == 0
        table += [(off + base, bs, seq_at, lseq) for off, bs, seq_at, lseq in recs]
    while True:                                                      # (a walk of three entries may have left records behind)
        recs, carry_from, err, _ = check_walk(chunk, chunk.mirror, carry_from, 1 << 16, "after the last fill")
        table += [(off + base, bs, seq_at, lseq) for off, bs, seq_at, lseq in recs]
        if not recs:
            break
    assert fed == len(stream) and base + carry_from == len(stream) and err == 0
    assert table == whole[0]
    for kind in ("none", "in place", "direct", "through the temporary"):
        assert moves.count(kind) >= 1, (kind, moves)
    assert moves[1:].count("none") >= 1
    assert moves == [m for m, _ in B.simulate_carry(stream, fills)]
    # refusals leave the chunk as it is
    size = chunk.size()
    comp, descs = B.pack_members(b"x" * 10, [10])
    assert size > 200 and chunk.inflate(comp, [(s, p, n, c, 99) for s, p, n, c, _ in descs], size - 100) == K.TS_ERR_INVALID_ARG
    assert chunk.inflate(comp, [(s, p, n, c, 0) for s, p, n, c, _ in descs], size - 1) == K.TS_ERR_INVALID_ARG
    assert chunk.inflate(comp, descs, size + 1) == K.TS_ERR_INVALID_ARG
    assert chunk.size() == size and chunk.read(0, size) == chunk.mirror
    assert chunk.fill(b"x" * 10, (comp, descs), size - 100) == chunk.mirror and chunk.size() == 110


# ================================================================================================================== gather
def gather_table(env, sizes, seed):
    gen = random.Random(seed)
    plain = env.chunk.fill_plain(b"".join(B.record_of_size(gen, s) for s in sizes))
    table, nxt, err, _ = check_walk(env.chunk, plain, 0, len(sizes) + 1, "gather table")
    assert (len(table), nxt, err) == (len(sizes), len(plain), 0) and [4 + t[1] for t in table] == list(sizes)
    return plain, table


def pass_patterns(n, seed):
    gen = random.Random(seed)
    pats = {"none": [0] * n, "all": [1] * n, "alternating": [i & 1 for i in range(n)], "alternating from 0": [1 - (i & 1) for i in range(n)],
            "first": [1] + [0] * (n - 1), "last": [0] * (n - 1) + [1],
            "random": [gen.choice((0, 0, 1, 255)) for _ in range(n)], "random, sparse": [int(gen.random() < 0.05) * 0x80 for _ in range(n)]}
    for k in (63, 64, 65):
        if k < n:
            pats["only %d" % k] = [int(i == k) for i in range(n)]
    return pats


def check_gather(env, plain, table, pats, what):
    import torch
    K, chunk = env.K, env.chunk
    for name, p in pats.items():
        exp, kept = B.ref_gather(plain, table, p)
        d_pass = torch.tensor(p, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rc, out, nbytes, npassed = chunk.gather(table, C.c_void_p(d_pass.data_ptr()), len(exp))     # cap == bytes
        assert (rc, nbytes, npassed) == (K.TS_OK, len(exp), kept), (what, name, rc, nbytes, npassed, len(exp), kept)
        assert_same_bytes(out, exp, "%s, %s" % (what, name))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 3000])
def test_gather_small_records(env, n):
    """Tables around the 64-record step of the prefix sum, each gathered with every pass pattern in turn from the same
    chunk (so every gather but the first follows one with other pass bytes)."""
    gen = random.Random(n)
    plain, table = gather_table(env, [gen.randrange(37, 300) for _ in range(n)], n)
    check_gather(env, plain, table, pass_patterns(n, n), "n = %d" % n)


@pytest.mark.parametrize("big", [{0: 70000}, {31: 65536}, {63: 200001}, {3: 66000, 4: 131077, 40: 65536 + 37, 63: 300000}],
                         ids=["step position 0", "step position 31", "step position 63", "four in one step"])
def test_gather_records_above_64k_among_small_ones(env, big):
    """The prefix sum adds a step's sizes in two 16-bit halves: records of more than 65 535 bytes in the second step of
    three, next to small ones."""
    gen = random.Random(len(big))
    sizes = [gen.randrange(37, 300) for _ in range(192)]
    for p, s in big.items():
        sizes[64 + p] = s
    assert min(big.values()) > 65535
    plain, table = gather_table(env, sizes, 5)
    pats = pass_patterns(192, 9)
    pats["only the large"] = [int(i - 64 in big) for i in range(192)]
    pats["all but the large"] = [int(i - 64 not in big) for i in range(192)]
    check_gather(env, plain, table, pats, "large at %r" % sorted(big))


def test_gather_capacity_and_seqless_records(env):
    import torch
    K, chunk = env.K, env.chunk
    gen = random.Random(21)
    recs = []
    for i in range(300):
        lseq = 0 if i % 4 == 1 else gen.randrange(1, 300)
        recs.append(B.build_record(1 + i % 7, i % 3, lseq, seq=bytes(gen.getrandbits(8) for _ in range((lseq + 1) // 2)), aux=gen.randrange(40)))
    plain = chunk.fill_plain(b"".join(recs))
    table = check_walk(chunk, plain, 0, 1000, "records with and without SEQ")[0]
    with_seq = [t for t in table if t[3]]
    assert len(table) == 300 and len(with_seq) == 225
    p = [gen.choice((0, 1)) for _ in with_seq]
    exp, kept = B.ref_gather(plain, with_seq, p)
    assert 50 < kept < 200
    # the pass bytes live in the chunk's own buffer here, as on the route
    d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, len(p))
    assert d_pass
    B.to_device(d_pass, bytes(p))
    rc, out, nbytes, npassed = chunk.gather(with_seq, d_pass, len(exp) - 1)
    assert (rc, nbytes, npassed) == (K.TS_ERR_INVALID_ARG, len(exp), kept)
    assert out == b"\xa5" * (len(exp) - 1)                                         # host_out untouched
    rc, out, nbytes, npassed = chunk.gather(with_seq, d_pass, len(exp) + 100)
    assert (rc, nbytes, npassed) == (K.TS_OK, len(exp), kept)
    assert_same_bytes(out[:len(exp)], exp, "gather of the records with SEQ")
    assert out[len(exp):] == b"\xa5" * 100
    rc, out, nbytes, npassed = chunk.gather(with_seq, d_pass, len(exp))
    assert (rc, nbytes, npassed, out) == (K.TS_OK, len(exp), kept, exp)
    # nothing passes, no room asked for
    B.to_device(d_pass, bytes(len(p)))
    assert chunk.gather(with_seq, d_pass, 0) == (K.TS_OK, b"", 0, 0)
    assert chunk.gather([], None, 0) == (K.TS_OK, b"", 0, 0)
    # other pass bytes from the same chunk, from a tensor
    q = [1 - x for x in p]
    t = torch.tensor(q, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    exp2, kept2 = B.ref_gather(plain, with_seq, q)
    assert chunk.gather(with_seq, C.c_void_p(t.data_ptr()), len(exp2)) == (K.TS_OK, exp2, len(exp2), kept2)
    # a table entry that does not lie in the chunk is refused on the host
    bad = list(with_seq)
    bad[7] = (chunk.size() - 10,) + bad[7][1:]
    rc, out, _, _ = chunk.gather(bad, C.c_void_p(t.data_ptr()), len(exp2))
    assert rc == K.TS_ERR_INVALID_ARG and out == b"\xa5" * len(exp2)
