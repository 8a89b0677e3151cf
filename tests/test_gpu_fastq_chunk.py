"""The stages of the device route of --fastq-subset, one by one through ctypes against the plain references of
tests/fastqchunk.py (pinned without a device by tests/test_fastq_chunk_reference_cpu.py): the walk's table, carry offset and
error triple; the staged sequences, byte for byte, with the zeros between and behind them; the gathered records with *bytes
and *n_passed; plain upload against BGZF members.  Equality is exact everywhere.  One context and one chunk serve the whole
module, reused across cases on purpose.  tests/test_gpu_fastq_device.py checks the route as a whole against the host route."""
import random
import types

import pytest

from tests import bamchunk as B
from tests import fastqchunk as F
from tests import harness as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("--fastq-subset -l 42")
    rf = ta.ReadTelomereFilter(user_input(opts, device=0))
    chunk = F.Chunk(rf._ctx.ptr, 64, 1 << 16)
    yield types.SimpleNamespace(K=K, L=K.lib(), rf=rf, ctx=rf._ctx.ptr, chunk=chunk)
    chunk.close()
    rf.close()


def check_walk(chunk, text, at_end, what=""):
    got, exp = chunk.fastq_walk(at_end, cap=max(16, len(text) // 8 + 16)), F.ref_walk(text, at_end)
    assert got[1:] == exp[1:], "%s: (next, error, error_record, error_off) %r, reference %r" % (what, got[1:], exp[1:])
    assert len(got[0]) == len(exp[0]), "%s: %d records, reference %d" % (what, len(got[0]), len(exp[0]))
    for i, (g, e) in enumerate(zip(got[0], exp[0])):
        assert g == e, "%s: record %d is %r, reference %r" % (what, i, g, e)
    return got


def feed(chunk, pieces):
    """The pieces one after the other, each behind what the walk before left unconsumed: every walk against the reference on
    the chunk's bytes; -> the records of all walks with offsets in the whole text, and the last walk's answer."""
    chunk.reset()
    nxt, base, table, got = 0, 0, [], None
    for k, piece in enumerate(pieces):
        held = len(chunk.mirror)
        text = chunk.upload(piece, nxt)
        base += nxt
        assert len(text) == held - nxt + len(piece)
        got = check_walk(chunk, text, k == len(pieces) - 1, "piece %d" % k)
        table += [(r[0] + base,) + r[1:] for r in got[0]]
        nxt = got[1]
    return table, got


@pytest.mark.parametrize("name", sorted(F.edge_cases()))
def test_walk_edge_cases(env, name):
    text = F.edge_cases()[name]
    for at_end in (True, False):
        env.chunk.reset()
        check_walk(env.chunk, env.chunk.upload(text, 0), at_end, name)


@pytest.mark.parametrize("name", sorted(F.error_cases()))
def test_walk_error_cases(env, name):
    text, kind, at = F.error_cases()[name]
    env.chunk.reset()
    got = check_walk(env.chunk, env.chunk.upload(text, 0), True, name)
    assert got[2:4] == (kind, at)
    env.chunk.reset()
    check_walk(env.chunk, env.chunk.upload(text, 0), False, name + ", not at the end")


def line_kinds_at(text, cuts):
    """Which of a record's four lines (0..3; 4: between records) each cut position falls in."""
    recs = F.ref_walk(text, True)[0]
    kinds = set()
    for c in cuts:
        for off, seq_at, seq_len, size, _ in recs:
            if off <= c <= off + size:
                kinds.add(text[off:c].count(b"\n"))
                break
        else:
            kinds.add(4)
    return kinds


@pytest.mark.parametrize("size", [37, 211, 1000, 4099, 16389])
@pytest.mark.parametrize("which", ["generated", "generated crlf"])
def test_walk_chunked_with_carry(env, which, size):
    """A text in pieces of `size` bytes: the tables of the chunks, put together, are the table of the whole text, whatever
    line of a record a piece ends in."""
    text = F.edge_cases()[which]
    cuts = list(range(size, len(text), size))
    if size <= 211:
        assert {0, 1, 2, 3} <= line_kinds_at(text, cuts)
    table, last = feed(env.chunk, [text[a:a + size] for a in range(0, len(text), size)])
    assert table == F.ref_walk(text, True)[0]
    assert last[1] == len(env.chunk.mirror) and last[2] == F.OK


def test_walk_blank_chunk_and_partial_record_chunks(env):
    a = F.record_text(b"first", b"TTAGGG" * 9)
    b = F.record_text(b"second with a long name " * 3, b"ACGT" * 20, qual=b"@" * 80)
    pieces = [a, b"\n\r\n\n", b"\n", b[:10], b[10:30], b[30:90], b[90:-1], b[-1:] + b"\n\n", a[:-1]]
    table, last = feed(env.chunk, pieces)
    whole = b"".join(pieces)
    assert table == F.ref_walk(whole, True)[0] and len(table) == 3
    # the chunk of blank lines alone holds no record and is consumed whole; a part of a record is carried whole
    env.chunk.reset()
    got = check_walk(env.chunk, env.chunk.upload(b"\n\r\n\n", 0), False, "blank lines only")
    assert got[0] == [] and got[1] == 4
    env.chunk.reset()
    got = check_walk(env.chunk, env.chunk.upload(b[:30], 0), False, "part of a record")
    assert got[0] == [] and got[1] == 0 and got[2] == F.OK


def test_walk_many_slices(env):
    """Texts of many 16 KB slices and of more than 64 slices of 2 048 lines: the scans across waves, with tiny records (the
    framing scan's worst case) and with a late error."""
    for seed, n, lo, hi in ((7, 5000, 20, 150), (8, 40000, 1, 6)):
        text = F.reads_text(seed, n, lo, hi)
        assert text.count(b"\n") > (64 * 2048 if n == 40000 else 8 * 2048) and len(text) > 20 * 16384
        env.chunk.reset()
        got = check_walk(env.chunk, env.chunk.upload(text, 0), True, "many slices %d" % seed)
        assert len(got[0]) == n
        cut = text[:len(text) - 3]
        env.chunk.reset()
        check_walk(env.chunk, env.chunk.upload(cut, 0), False, "many slices %d, cut" % seed)
    recs = F.ref_walk(text, True)[0]
    bad = bytearray(text)
    bad[recs[39000][0]] = ord("X")
    bad[recs[39500][0]] = ord("Y")
    env.chunk.reset()
    got = check_walk(env.chunk, env.chunk.upload(bytes(bad), 0), True, "late error")
    assert got[2:4] == (F.BAD_HEADER, 39000)
    # a table that is too small: INVALID_ARG, *n says what is needed, the table's first entries are filled
    import ctypes as C
    K = env.K
    arr = (K.FastqRecord * 10)()
    n_, nxt, err, erec, eoff = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint64(), C.c_uint64()
    env.chunk.reset()
    env.chunk.upload(text, 0)
    rc = env.L.ts_fastq_chunk_walk(env.chunk.ptr, 1, arr, 10, C.byref(n_), C.byref(nxt), C.byref(err), C.byref(erec), C.byref(eoff))
    assert rc == K.TS_ERR_INVALID_ARG and n_.value == 40000 and (arr[9].off, arr[9].size) == (recs[9][0], recs[9][3])


def stage_text():
    """Reads of every length around the 16-byte stores and the 8 192-byte pieces, behind names of every length mod 16 (the
    sequence starts at every alignment), some with CR LF."""
    gen = random.Random(21)
    lengths = list(range(1, 50)) + [8175, 8176, 8177, 8191, 8192, 8193, 8207, 8208, 8209, 16384, 16385, 40001]
    out = []
    for i, n in enumerate(lengths):
        eol = b"\r\n" if i % 7 == 3 else b"\n"
        out.append(F.record_text(b"n" * (1 + i % 16) + b"%d" % (i % 10), F.random_read(gen, n, telomeric=i % 4 == 0), eol=eol))
        if i % 9 == 4:
            out.append(F.record_text(b"nobases", b"", eol=eol))
    return b"".join(out), lengths


def test_stage_every_length_and_alignment(env):
    text, lengths = stage_text()
    chunk = env.chunk
    chunk.reset()
    recs = check_walk(chunk, chunk.upload(text, 0), True, "stage text")[0]
    with_seq = [r for r in recs if r[2] > r[4]]
    assert [r[2] - r[4] for r in with_seq] == lengths and len(recs) > len(with_seq)
    assert {(r[0] + r[1]) % 16 for r in with_seq} == set(range(16))
    reads = [F.ref_sequence(text, r) for r in with_seq]
    assert all(b"\r" not in r and b"\n" not in r for r in reads)
    batch = B.ReadBatch(env.ctx, lengths)
    try:
        for _ in range(2):                                          # (the second time into a buffer that holds the first)
            assert chunk.stage(with_seq, batch.ptr) == env.K.TS_OK, env.L.ts_last_error(env.ctx)
            assert all(o % 16 == 0 for o in batch.offsets)
            got, exp = batch.image(), batch.expected_image(reads)
            assert len(got) == len(exp)
            if got != exp:
                at = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
                raise AssertionError("input buffer differs first at byte %d: %r, expected %r" % (at, got[at:at + 16], exp[at:at + 16]))
        # a record without bases, or a segment of another length, is refused
        one = B.ReadBatch(env.ctx, [1])
        assert chunk.stage([r for r in recs if r[2] == r[4]][:1], one.ptr) == env.K.TS_ERR_INVALID_ARG
        one.close()
    finally:
        batch.close()


def test_gather_pass_vectors(env):
    """All, none and seeded random pass vectors over the stage text (records of 1 byte to 40 KB of sequence at every
    alignment) and over short reads: the passing records' four lines and a newline each, in input order."""
    chunk = env.chunk
    for text in (stage_text()[0], F.reads_text(5, 700)):
        chunk.reset()
        recs = check_walk(chunk, chunk.upload(text, 0), True, "gather text")[0]
        n = len(recs)
        d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, n)
        assert d_pass
        gen = random.Random(n)
        vectors = [bytes([1]) * n, bytes(n)] + [bytes(gen.choice((0, 1, 0, 255)) for _ in range(n)) for _ in range(4)] + \
                  [bytes(1 if i == k else 0 for i in range(n)) for k in (0, n - 1)]
        for v in vectors:
            B.to_device(d_pass, v)
            exp, kept = F.ref_gather(text, recs, v)
            rc, out, nbytes, npassed = chunk.fastq_gather(recs, d_pass, len(exp) + 64)
            assert rc == env.K.TS_OK, env.L.ts_last_error(env.ctx)
            assert (nbytes, npassed) == (len(exp), kept)
            assert out[:nbytes] == exp and out[nbytes:] == b"\xa5" * 64
        B.to_device(d_pass, vectors[0])
        exp, kept = F.ref_gather(text, recs, vectors[0])
        rc, out, nbytes, npassed = chunk.fastq_gather(recs, d_pass, len(exp) - 1)
        assert rc == env.K.TS_ERR_INVALID_ARG and (nbytes, npassed) == (len(exp), kept) and out == b"\xa5" * (len(exp) - 1)


def test_plain_upload_and_bgzf_members_agree(env):
    """The same text fed by plain upload and as BGZF members (stored and deflated, in pieces with a carry): equal chunks, equal
    tables, equal gathered bytes."""
    text = F.reads_text(9, 900)
    big = F.Chunk(env.ctx, 1 << 20, 1 << 20)
    try:
        plain_table, _ = feed(env.chunk, [text[a:a + 70000] for a in range(0, len(text), 70000)])
        nxt, base, table = 0, 0, []
        pieces = [text[a:a + 70000] for a in range(0, len(text), 70000)]
        for k, piece in enumerate(pieces):
            held = big.fill(piece, B.members_of(piece, 30011, "zlib" if k % 2 else "stored"), nxt)
            base += nxt
            got = check_walk(big, held, k == len(pieces) - 1, "members %d" % k)
            table += [(r[0] + base,) + r[1:] for r in got[0]]
            nxt = got[1]
        assert table == plain_table == F.ref_walk(text, True)[0]
        # the whole text in both chunks: gathered bytes
        env.chunk.reset()
        env.chunk.upload(text, 0)
        big.reset()
        big.fill(text, B.members_of(text, 65280, "zlib"))
        recs = plain_table
        v = bytes(i % 3 == 0 for i in range(len(recs)))
        outs = []
        for ch in (env.chunk, big):
            d_pass = env.L.ts_bam_chunk_pass_buffer(ch.ptr, len(recs))
            B.to_device(d_pass, v)
            rc, out, nbytes, npassed = ch.fastq_gather(recs, d_pass, len(text) + len(recs))
            assert rc == env.K.TS_OK
            outs.append(out[:nbytes])
        assert outs[0] == outs[1] == F.ref_gather(text, recs, v)[0]
    finally:
        big.close()


def test_chunk_grows_and_keeps_what_it_holds(env):
    small = F.Chunk(env.ctx, 64, 100)
    try:
        text = F.reads_text(12, 60)
        small.upload(text[:90], 0)
        small.upload(text[90:5000], 0)                                  # (everything carried: the chunk grows)
        small.upload(text[5000:], 10)
        assert small.mirror == text[10:]
        assert env.L.ts_chunk_reserve(small.ptr, 1 << 20) == env.K.TS_OK
        assert small.read(0, len(small.mirror)) == text[10:]
    finally:
        small.close()
