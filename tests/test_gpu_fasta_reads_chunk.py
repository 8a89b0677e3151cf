"""The stages of the device route of the FASTA read subset, one by one through ctypes against the plain references of
tests/fastareads.py (pinned without a device by tests/test_fasta_reads_reference_cpu.py): ts_fasta_chunk_stage — the batch's whole
input buffer image, the zeros between and behind the reads included —, ts_fasta_chunk_gather and ts_fasta_chunk_block_lines, on a
tiled tips batch (-l 42) and on a general one (-p TTAGGG,TTAGG).  The verdicts in between are the CPU oracle's.  Equality is exact
everywhere.  The shapes are the smallest at which the stage can go wrong: bodies without bases and without a final newline, line
widths around the 16-byte rows with LF and CR LF, read lengths around a row, a read that crosses a 16 KB slice of body text
unwrapped and as one-base CR LF lines in every phase, sub-tables of a walk, and a record carried into another chunk.  One
context and one chunk per batch kind serve the whole module, reused across cases on purpose."""
import ctypes as C
import random
import types

import pytest

from tests import bamchunk as B
from tests import fastachunk as F
from tests import fastareads as R
from tests import readblocks as RB
from tests import readsets

pytestmark = pytest.mark.gpu
SLICE = 16384                                                       # kFastaSliceBytes
KINDS = {"tiled": "-l 42", "general": readsets.SETS[0]}


@pytest.fixture(scope="module", params=sorted(KINDS))
def env(request):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    from tests.backends import OracleReadFilter
    flags = KINDS[request.param]
    rf = ta.ReadTelomereFilter(user_input(readsets.options(flags), device=0))
    assert bool(K.lib().ts_uses_fast_path(rf._ctx.ptr)) == (request.param == "tiled")
    chunk = R.Chunk(rf._ctx.ptr, 64, 1 << 16)
    yield types.SimpleNamespace(K=K, L=K.lib(), rf=rf, ctx=rf._ctx.ptr, chunk=chunk, judge=OracleReadFilter(readsets.options(flags)),
                                oracle=RB.read_oracle(flags))
    chunk.close()
    rf.close()


def first_difference(got, exp):
    return next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))


def walk(env, text, at_end, what):
    """The chunk's contents (`text`) walked: the table must be the reference's."""
    exp = F.ref_walk(text, at_end)
    rc, recs, nxt, _, n, _ = env.chunk.fasta_walk(at_end, cap=len(exp[0]) + 4, names_cap=len(exp[2]) + 16)
    assert rc == env.K.TS_OK, env.L.ts_last_error(env.ctx)
    assert (recs, nxt) == (exp[0], exp[1]), what
    return recs


def check_stages(env, text, recs, at_end, what):
    """Stage, judge, gather and block lines of `recs` (entries of the chunk's walk, in any selection) against the references."""
    K, L, chunk = env.K, env.L, env.chunk
    n = len(recs)
    reads = [F.ref_bases(text, r, at_end) for r in recs]
    batch = B.ReadBatch(env.ctx, [len(r) for r in reads])
    try:
        for _ in range(2):                                          # (the second time into a buffer that holds the first)
            assert chunk.reads_stage(recs, at_end, batch.ptr) == K.TS_OK, L.ts_last_error(env.ctx)
            assert all(o % 16 == 0 for o in batch.offsets)
            got, exp = batch.image(), R.ref_stage(batch.offsets, batch.input_bytes, text, recs, at_end)
            assert len(got) == len(exp)
            if got != exp:
                at = first_difference(got, exp)
                raise AssertionError("%s: the input buffer differs first at byte %d of %d: %r, expected %r" % (what, at, len(exp), got[at:at + 16], exp[at:at + 16]))
        d_pass = L.ts_bam_chunk_pass_buffer(chunk.ptr, n)
        assert d_pass
        assert L.ts_batch_scan(batch.ptr, None, None) == K.TS_OK, L.ts_last_error(env.ctx)
        flag = C.c_int(7)
        assert L.ts_batch_read_pass(batch.ptr, d_pass, None) == K.TS_OK, L.ts_last_error(env.ctx)
        assert L.ts_batch_read_pass_status(batch.ptr, C.byref(flag)) == K.TS_OK and flag.value == 0
        passes = [1 if p else 0 for p in env.judge.filter(reads)]
        assert list(B.device_bytes(d_pass, n)) == passes, what
        # the gather under the verdicts
        exp, kept = R.ref_gather(text, recs, passes)
        rc, out, nbytes, npassed = chunk.reads_gather(recs, d_pass, len(exp) + 64)
        assert rc == K.TS_OK, L.ts_last_error(env.ctx)
        assert (nbytes, npassed) == (len(exp), kept) and out[:nbytes] == exp and out[nbytes:] == b"\xa5" * 64, what
        # the block report of the kept reads
        assert L.ts_batch_call_read_blocks(batch.ptr, None) == K.TS_OK, L.ts_last_error(env.ctx)
        assert L.ts_batch_read_pass_status(batch.ptr, C.byref(flag)) == K.TS_OK and flag.value == 0
        # (the filter folds case before it scans, as the oracle's read filter does; the oracle's segment scan is given the folded read)
        exp, with_lines = RB.ref_report(list(zip(R.ref_names(text, recs), [r.upper() for r in reads])), env.oracle)
        assert len(with_lines) == kept
        rc, out, nbytes, nlines = chunk.reads_block_lines(recs, batch.ptr, len(exp) + 16)
        assert rc == K.TS_OK, L.ts_last_error(env.ctx)
        assert (nbytes, nlines) == (len(exp), exp.count(b"\n")) and out[:nbytes] == exp and out[nbytes:] == b"\x5a" * 16, what
        if exp:                                                     # too small: nothing is copied, *bytes says what is needed
            rc, out, nbytes, _ = chunk.reads_block_lines(recs, batch.ptr, len(exp) - 1)
            assert rc == K.TS_ERR_INVALID_ARG and nbytes == len(exp) and out == b"\x5a" * (len(exp) - 1)
        return kept
    finally:
        batch.close()


def check_gather_all(env, text, recs, what):
    """Every record of the table, those without bases too, under a pass vector of ones, of every other one and of none."""
    K, L, chunk = env.K, env.L, env.chunk
    n = len(recs)
    d_pass = L.ts_bam_chunk_pass_buffer(chunk.ptr, max(n, 1))
    assert d_pass
    for v in (bytes([1]) * n, bytes(i % 2 for i in range(n)), bytes((i + 1) % 2 * 255 for i in range(n)), bytes(n)):
        B.to_device(d_pass, v)
        exp, kept = R.ref_gather(text, recs, v)
        rc, out, nbytes, npassed = chunk.reads_gather(recs, d_pass, len(exp) + 64)
        assert rc == K.TS_OK, L.ts_last_error(env.ctx)
        assert (nbytes, npassed) == (len(exp), kept) and out[:nbytes] == exp and out[nbytes:] == b"\xa5" * 64, what


def check_text(env, text, what, at_end=True, select=None):
    """Upload, walk, and the stages over the records with bases (or over select(those)); -> (the table, records kept)"""
    env.chunk.reset()
    recs = walk(env, env.chunk.upload(text, 0), at_end, what)
    check_gather_all(env, text, recs, what)
    with_seq = [r for r in recs if r[3] > 0]
    if select:
        with_seq = select(with_seq)
    kept = check_stages(env, text, with_seq, at_end, what) if with_seq else 0
    return recs, kept


def read_of(gen, n, telomeric):
    """n bases: telomere repeats in front (all of a short read) or random bases."""
    body = bytes(gen.choice(b"ACGT") for _ in range(n))
    return ((b"TTAGGG" * 40)[:min(n, 240)] + body[min(n, 240):]) if telomeric else body


@pytest.mark.parametrize("name", sorted(R.edge_cases()))
def test_edge_cases(env, name):
    """Bodies of no lines and of blank lines only, a last line without its newline, a '\\r' as the input's last byte, a '>' inside
    a body line, names that are empty, hold a space or a tab or are 300 bytes long, and line widths 1, 15, 16, 17, 60 and 61 with
    LF and CR LF."""
    text = R.edge_cases()[name]
    recs, kept = check_text(env, text, name)
    if any(r[3] >= 54 for r in recs):
        assert kept > 0, name                                       # (the telomeric reads of the cases are kept: the report has lines)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_read_lengths_around_a_row(env, eol):
    """Reads of n % 16 == 0, 1 and 15 (and of 1 to 17 bases), unwrapped and at widths that are and are not multiples of 16, their
    bodies at every address mod 16."""
    gen = random.Random(3)
    lengths = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 240, 241, 255, 256, 257]
    body_at = set()
    for width in (None, 16, 60):
        reads, names = [], []
        for k in range(16):
            for n in lengths[k % 4::4]:
                reads.append(read_of(gen, n, len(reads) % 2 == 0))
                names.append(b"n" * (1 + (k + len(reads)) % 16))
        text = R.reads_text(reads, width, eol, names)
        recs, kept = check_text(env, text, "lengths, width %r" % width)
        body_at |= {(r[0] + r[2]) % 16 for r in recs}
        assert {r[3] % 16 for r in recs} >= {0, 1, 15} and 0 < kept < len(recs)
    assert body_at == set(range(16))


def test_an_unwrapped_read_across_a_slice(env):
    """One body line of 20 000 bases: two jobs, the second one's place is the first one's count; its neighbours lie in one
    slice each."""
    gen = random.Random(5)
    reads = [read_of(gen, 300, True), read_of(gen, 20000, True), read_of(gen, 301, False), read_of(gen, 20000, False), read_of(gen, 17, True)]
    for eol in (b"\n", b"\r\n"):
        text = R.reads_text(reads, None, eol)
        recs, kept = check_text(env, text, "20 000 bases unwrapped")
        assert [r[0] // SLICE != (r[0] + r[1] - 1) // SLICE for r in recs] == [False, True, False, True, False] and kept == 2


@pytest.mark.parametrize("name_len", [5, 6, 7])
def test_one_base_crlf_lines_across_slices(env, name_len):
    """A read of 12 000 lines of one base and CR LF: 36 000 body bytes over three slices, whose boundaries fall between a base and
    its '\\r', between '\\r' and '\\n' and behind the '\\n' — names of three consecutive lengths shift the body through every phase."""
    gen = random.Random(7)
    reads = [read_of(gen, 100, False), read_of(gen, 12000, True), read_of(gen, 100, True)]
    texts = {k: R.reads_text(reads, 1, b"\r\n", [b"a", b"b" * k, b"c"]) for k in (5, 6, 7)}
    # (which byte of a line a slice begins with: all three across the three texts, and across the two boundaries of each)
    assert {(SLICE - (F.ref_walk(t, True)[0][1][0] + F.ref_walk(t, True)[0][1][2])) % 3 for t in texts.values()} == {0, 1, 2}
    recs, kept = check_text(env, texts[name_len], "one-base crlf lines")
    assert recs[1][3] == 12000 and recs[1][1] == len(b">" + b"b" * name_len + b"\r\n") + 36000 and kept == 2
    # ... and without the '\r': lines of two bytes
    check_text(env, R.reads_text(reads, 1, b"\n", [b"a", b"b" * name_len, b"c"]), "one-base lf lines")


def test_sub_tables(env):
    """Every third record of a walk, a single record in one slice and a single one across slices, and the table in reverse: the
    stage takes any entries of the last walk's table, not only recs[0, n)."""
    gen = random.Random(11)
    reads = [read_of(gen, [40, 700, 20000, 97, 1, 16][i % 6], i % 2 == 0) for i in range(24)]
    text = R.reads_text(reads, 61, b"\r\n")
    for what, select in (("every third", lambda t: t[::3]), ("every third from 2", lambda t: t[2::3]), ("one short", lambda t: t[3:4]),
                         ("one long", lambda t: t[8:9]), ("reversed", lambda t: t[::-1])):
        recs, _ = check_text(env, text, what, select=select)
    assert len(recs) == 24
    # what the stage refuses: a record without bases, a segment of another length, a record that leaves the chunk
    K, chunk = env.K, env.chunk
    text = b">a\n>b\nACGT\nAC\n"
    chunk.reset()
    recs = walk(env, chunk.upload(text, 0), True, "refusals")
    one, six = B.ReadBatch(env.ctx, [1]), B.ReadBatch(env.ctx, [6])
    try:
        assert chunk.reads_stage(recs[1:], True, six.ptr) == K.TS_OK
        assert chunk.reads_stage(recs[:1], True, one.ptr) == K.TS_ERR_INVALID_ARG
        assert chunk.reads_stage(recs[1:], True, one.ptr) == K.TS_ERR_INVALID_ARG
        outside = [(recs[1][0], recs[1][1] + 1) + recs[1][2:]]
        assert chunk.reads_stage(outside, True, six.ptr) == K.TS_ERR_INVALID_ARG
        d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, 1)
        assert chunk.reads_gather(outside, d_pass, 4096)[0] == K.TS_ERR_INVALID_ARG
        assert chunk.reads_block_lines(outside, six.ptr, 4096)[0] == K.TS_ERR_INVALID_ARG
    finally:
        one.close()
        six.close()


def test_a_record_carried_into_another_chunk(env):
    """Walked with at_end = 0 the chunk's last record is open: its whole records are staged and gathered (a '\\r' at the chunk's end
    is not the input's), the open one is carried into another chunk, the rest of the text goes behind it, and the second walk's
    records give the rest of the subset."""
    gen = random.Random(13)
    reads = [read_of(gen, n, i in (0, 2, 3)) for i, n in enumerate([500, 3000, 64, 20000, 33, 900])]
    text = R.reads_text(reads, 60, b"\r\n", last_eol=False) + b"\r"
    whole = F.ref_walk(text, True)[0]
    a, b = env.chunk, R.Chunk(env.ctx, 64, 256)
    try:
        for cut in (whole[3][0] + whole[3][2] + 9000, whole[4][0] - 1, len(text) - 1):
            a.reset()
            head = walk(env, a.upload(text[:cut], 0), False, "head")
            nxt = F.ref_walk(text[:cut], False)[1]
            assert 0 < nxt < cut and head == whole[:len(head)]
            kept = check_stages(env, text[:cut], head, False, "head")
            assert env.L.ts_chunk_carry_over(b.ptr, a.ptr, nxt, None) == env.K.TS_OK, env.L.ts_last_error(env.ctx)
            b.mirror = text[nxt:cut]
            rest_text = b.upload(text[cut:], 0)
            assert rest_text == text[nxt:]
            env.chunk = b
            try:
                rest = walk(env, rest_text, True, "the carried record and what follows")
                assert [(r[0] + nxt,) + r[1:4] for r in rest] == [r[:4] for r in whole[len(head):]]
                kept += check_stages(env, rest_text, rest, True, "rest")
            finally:
                env.chunk = a
            assert kept == 3
    finally:
        b.close()
