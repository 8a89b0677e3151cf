"""ts_bam_chunk_gather_fastq and ts_sam_chunk_gather_fastq (read_fastq.hip) through ctypes against the plain-Python rule of
tests/readfastq.py, byte for byte, with host_out exact and one byte short.  The shapes are the smallest at which the kernels can
go wrong: L around the 16 bytes of a store and around one and two pieces of the job list, each forward and reversed (the odd
nibble phase and the last half byte of a packed SEQ); a text that starts on each of the 16 store phases; a record first and last in
a chunk that is exactly as large as its bytes; no, every and every other pass byte; missing and saturating QUAL; SAM lines with
CR LF and lines that end at a tab; and a fixed-seed mix of 2 000 short records.  One context and one chunk serve the module."""
import ctypes as C
import random
import subprocess
import types

import pytest

from tests import bamchunk as B
from tests import harness as H
from tests import readfastq as Q
from tests import samchunk as S

pytestmark = pytest.mark.gpu
R = Q.RESTORE_STRAND


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("--fastq-subset -l 42")
    rf = ta.ReadTelomereFilter(user_input(opts, device=0))
    chunk = S.Chunk(rf._ctx.ptr, 64, 1 << 16)
    yield types.SimpleNamespace(K=K, L=K.lib(), rf=rf, ctx=rf._ctx.ptr, chunk=chunk)
    chunk.close()
    rf.close()


@pytest.fixture(scope="module")
def piece():
    """The device piece size, from the host program's --constants (the core header's named constant)."""
    import os
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "host")
        subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "read_fastq_format_host.cpp"), "-o", exe])
        out = subprocess.run([exe, "--constants"], capture_output=True, timeout=60, check=True).stdout.split()
    assert out[0] == b"piece_bytes"
    return int(out[1])


def bam_table(records):
    """BAM records back to back -> (the bytes, the (off, block_size, seq_at, l_seq) table)"""
    table, off = [], 0
    for r in records:
        table.append((off, len(r) - 4, 36 + r[12] + 4 * int.from_bytes(r[16:18], "little"), int.from_bytes(r[20:24], "little")))
        off += len(r)
    return b"".join(records), table


def sam_table(lines):
    """SAM lines with their line ends (the last may lack its '\\n') -> (the bytes, the (off, seq_at, seq_len, size, flags) table)"""
    table, off = [], 0
    for ln in lines:
        content = ln[:-1] if ln.endswith(b"\n") else ln
        f = content.split(b"\t")
        seq_at = sum(len(x) + 1 for x in f[:9])
        table.append((off, seq_at, len(f[9]), len(content), 1 if f[9] == b"*" else 0))
        off += len(ln)
    return b"".join(lines), table


def gather(env, kind, chunk, table, d_pass, flags, cap, fill=0xA5):
    out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
    nbytes, npassed = C.c_uint64(0xdead), C.c_uint64(0xdead)
    if kind == "B":
        rc = env.L.ts_bam_chunk_gather_fastq(chunk.ptr, B.table_of(table), len(table), d_pass, flags, out, cap, C.byref(nbytes), C.byref(npassed), None)
    else:
        rc = env.L.ts_sam_chunk_gather_fastq(chunk.ptr, S.table_of(table), len(table), d_pass, flags, out, cap, C.byref(nbytes), C.byref(npassed), None)
    return rc, (out.raw if cap else b""), nbytes.value, npassed.value


def check(env, kind, records, passes=None, chunk=None, flag_values=(0, R)):
    """The records in one chunk, gathered under `passes` (default: all) with each value of `flags`: the Python rule's text of the
    passing records, exactly; then a host_out one byte short: nothing is copied."""
    chunk = chunk or env.chunk
    text, table = (bam_table if kind == "B" else sam_table)(records)
    chunk.reset()
    chunk.upload(text, 0)
    n = len(records)
    passes = bytes([1]) * n if passes is None else passes
    d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, max(n, 1))
    assert d_pass
    B.to_device(d_pass, passes)
    for flags in flag_values:
        exp = b"".join((Q.bam_text if kind == "B" else Q.sam_text)(r, flags) for r, p in zip(records, passes) if p)
        kept = sum(1 for p in passes if p)
        rc, out, nbytes, npassed = gather(env, kind, chunk, table, d_pass, flags, len(exp) + 64)
        assert rc == env.K.TS_OK, env.L.ts_last_error(env.ctx)
        assert (nbytes, npassed) == (len(exp), kept)
        if out[:nbytes] != exp:
            at = next(i for i, (a, b) in enumerate(zip(out, exp)) if a != b)
            raise AssertionError("%s flags %d: the text differs first at byte %d of %d: %r, expected %r" % (kind, flags, at, len(exp), out[max(0, at - 8):at + 24], exp[max(0, at - 8):at + 24]))
        assert out[nbytes:] == b"\xa5" * 64
        rc, out, nbytes, npassed = gather(env, kind, chunk, table, d_pass, flags, len(exp))            # exact
        assert rc == env.K.TS_OK and out == exp
        if exp:
            rc, out, nbytes, npassed = gather(env, kind, chunk, table, d_pass, flags, len(exp) - 1)     # one short
            assert rc == env.K.TS_ERR_INVALID_ARG and (nbytes, npassed) == (len(exp), kept) and out == b"\xa5" * (len(exp) - 1)


def bam_of(rng, name, flag, n, qual="random"):
    codes = [rng.randrange(16) for _ in range(n)]
    q = None if qual is None else [rng.randrange(0, 94) for _ in range(n)] if qual == "random" else qual
    return Q.bam_record(name, flag, codes, q, n_cigar=rng.randrange(3), tail=bytes(rng.randrange(256) for _ in range(rng.randrange(6))))


SAM_ALPHABET = b"ACGTNacgtnUuMRWSYKVHDBmrwsykvhdb=."


def sam_of(rng, name, flag, n, qual="random", tags=None, eol=b"\n"):
    seq = bytes(rng.choice(SAM_ALPHABET) for _ in range(n))
    q = b"*" if qual is None else bytes(rng.randrange(33, 127) for _ in range(n)) if qual == "random" else qual
    if n == 1 and q == b"*" and qual is not None:
        q = b"I"
    return Q.sam_line(name, flag, seq, q, tags=tags, eol=eol)


def lengths(piece):
    return [1, 2, 15, 16, 17, 31, 32, 33, piece - 1, piece, piece + 1, 2 * piece + 1]


@pytest.mark.parametrize("kind", ["B", "S"])
def test_lengths_around_a_store_and_a_piece_forward_and_reversed(env, piece, kind):
    rng = random.Random(3)
    records = []
    for n in lengths(piece):
        for flag in (0, 16):
            if kind == "B":
                records.append(bam_of(rng, b"L%d" % n, flag, n))
            else:
                records.append(sam_of(rng, b"L%d" % n, b"%d" % flag, n, tags=[None, b"NM:i:0"][n & 1]))
    check(env, kind, records)
    # ... and each alone in the chunk, so that every length meets the chunk's first byte and its last
    for rec in records:
        check(env, kind, [rec], flag_values=(R,))


@pytest.mark.parametrize("kind", ["B", "S"])
def test_text_starts_on_every_store_phase(env, kind):
    """A record of name length 0, 1 ... 16 and 254 in front of one fixed record: its text starts at byte name_len + 16."""
    rng = random.Random(4)
    fixed = bam_of(rng, b"fixed", 16, 100) if kind == "B" else sam_of(rng, b"fixed", b"16", 100)
    for nl in list(range(17)) + [254]:
        name = bytes(33 + (7 * i + nl) % 94 for i in range(nl))
        front = bam_of(rng, name, 0, 5) if kind == "B" else sam_of(rng, name, b"0", 5)
        exp_front = (Q.bam_text if kind == "B" else Q.sam_text)(front, R)
        assert len(exp_front) == nl + 16
        check(env, kind, [front, fixed, front], flag_values=(R,))
        check(env, kind, [front, fixed, front], passes=bytes([0, 1, 0]), flag_values=(R,))


@pytest.mark.parametrize("kind", ["B", "S"])
def test_first_and_last_record_of_a_chunk_of_exactly_their_size(env, piece, kind):
    """The chunk's capacity is the bytes it holds: the first record starts at its base (the backward reads of the reverse form
    stop there) and the last ends at its capacity (the forward reads run into the 64 readable bytes behind it)."""
    rng = random.Random(6)
    for n in (1, 16, 33, piece + 1):
        if kind == "B":
            records = [bam_of(rng, b"", 16, n), bam_of(rng, b"mid", 0, 7), Q.bam_record(b"z", 16, [rng.randrange(16) for _ in range(n)], [rng.randrange(94) for _ in range(n)])]
        else:
            records = [sam_of(rng, b"", b"16", n), sam_of(rng, b"mid", b"0", 7), sam_of(rng, b"z", b"16", n, eol=b"")]
        size = sum(len(r) for r in records)
        chunk = S.Chunk(env.ctx, 64, size)
        try:
            check(env, kind, records, chunk=chunk)
            check(env, kind, records, passes=bytes([1, 0, 1]), chunk=chunk)
            assert chunk.size() == size
        finally:
            chunk.close()


def test_missing_and_saturating_qual(env):
    rng = random.Random(8)
    bam = [bam_of(rng, b"m%d" % n, f, n, qual=None) for n in (1, 5, 16, 40) for f in (0, 16)]
    bam += [bam_of(rng, b"s%d" % n, f, n, qual=[(92, 93, 94, 127, 128, 200, 254, 255, 0)[(i + n) % 9] if i else 93 for i in range(n)]) for n in (3, 16, 35, 64) for f in (0, 16)]
    check(env, "B", bam)
    sam = [sam_of(rng, b"m%d" % n, f, n, qual=None, tags=t) for n in (2, 5, 16, 40) for f in (b"0", b"16") for t in (None, b"XX:i:1")]
    sam += [Q.sam_line(b"one", b"16", b"a", b"*"), Q.sam_line(b"one", b"0", b"C", b"*", tags=b"NM:i:0"), Q.sam_line(b"star", b"16", b"AC", b"**")]
    check(env, "S", sam)


def test_sam_crlf_lines_and_lines_that_end_at_a_tab(env):
    rng = random.Random(9)
    lines = []
    for n in (1, 3, 16, 17, 50):
        for flag in (b"16", b"0", b"0016", b"x", b"", b"1040"):
            lines.append(sam_of(rng, b"c%d" % n, flag, n, eol=b"\r\n"))
            lines.append(sam_of(rng, b"t%d" % n, flag, n, tags=b""))
            lines.append(sam_of(rng, b"ct%d" % n, flag, n, tags=b"", eol=b"\r\n"))
            lines.append(sam_of(rng, b"q%d" % n, flag, n, qual=None, eol=b"\r\n"))
    lines.append(sam_of(rng, b"last", b"16", 21, eol=b"\r"))       # the input's last line, without its '\n'
    check(env, "S", lines)


@pytest.mark.parametrize("kind", ["B", "S"])
def test_pass_vectors_on_a_mix_of_2000_short_records(env, kind):
    rng = random.Random(12)
    records = []
    for i in range(2000):
        n = rng.choice([1, 2, 3, 7, 15, 16, 17, 30, 31, 32, 33, 64, 100, 151, 300])
        name = bytes(rng.randrange(33, 127) for _ in range(rng.choice([0, 1, 5, 12, 20, 40])))
        missing = rng.random() < 0.2
        if kind == "B":
            records.append(bam_of(rng, name, rng.choice([0, 4, 16, 20, 0x910, 0x900]), n, qual=None if missing else "random"))
        else:
            records.append(sam_of(rng, name, rng.choice([b"0", b"4", b"16", b"20", b"2320", b"2304"]), n, qual=None if missing else "random",
                                  tags=rng.choice([None, b"NM:i:0", b""]), eol=rng.choice([b"\n", b"\n", b"\r\n"])))
    n = len(records)
    check(env, kind, records, passes=bytes(n))
    check(env, kind, records)
    check(env, kind, records, passes=bytes(i % 2 for i in range(n)), flag_values=(R,))
    check(env, kind, records, passes=bytes((i + 1) % 2 * 255 for i in range(n)), flag_values=(R,))


def test_arguments_and_statistics(env):
    rng = random.Random(13)
    records = [bam_of(rng, b"a", 16, 20), bam_of(rng, b"b", 0, 30)]
    text, table = bam_table(records)
    chunk = env.chunk
    chunk.reset()
    chunk.upload(text, 0)
    d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, 2)
    B.to_device(d_pass, b"\x01\x01")
    before = (C.c_uint64 * 3)()
    assert env.L.ts_read_fastq_text_stats(env.ctx, before) == env.K.TS_OK
    exp = b"".join(Q.bam_text(r, R) for r in records)
    rc, out, nbytes, npassed = gather(env, "B", chunk, table, d_pass, R, len(exp))
    assert rc == env.K.TS_OK and out == exp
    after = (C.c_uint64 * 3)()
    assert env.L.ts_read_fastq_text_stats(env.ctx, after) == env.K.TS_OK
    assert [a - b for a, b in zip(after, before)] == [1, 2, len(exp)]
    # an unknown flag bit, and a record whose QUAL leaves it or that leaves the chunk, are refused
    assert gather(env, "B", chunk, table, d_pass, 2, 4096)[0] == env.K.TS_ERR_INVALID_ARG
    assert gather(env, "B", chunk, [(table[0][0], table[0][1], table[0][2] + len(records[0]), table[0][3])], d_pass, R, 4096)[0] == env.K.TS_ERR_INVALID_ARG
    assert gather(env, "B", chunk, [(table[1][0], table[1][1] + 1, table[1][2], table[1][3])], d_pass, R, 4096)[0] == env.K.TS_ERR_INVALID_ARG
    lines = [sam_of(rng, b"s", b"16", 9)]
    text, stable = sam_table(lines)
    chunk.reset()
    chunk.upload(text, 0)
    assert gather(env, "S", chunk, stable, d_pass, 4, 4096)[0] == env.K.TS_ERR_INVALID_ARG
    assert gather(env, "S", chunk, [(0, stable[0][1], stable[0][2], stable[0][3] + 2, 0)], d_pass, R, 4096)[0] == env.K.TS_ERR_INVALID_ARG
    # nothing to do: no record, no text, no call counted
    rc, out, nbytes, npassed = gather(env, "S", chunk, [], None, R, 0)
    assert rc == env.K.TS_OK and (nbytes, npassed) == (0, 0)
    last = (C.c_uint64 * 3)()
    assert env.L.ts_read_fastq_text_stats(env.ctx, last) == env.K.TS_OK and list(last) == list(after)
