"""The stages of the device route of --sam-subset, one by one through ctypes against the plain references of tests/samchunk.py
(pinned without a device by tests/test_sam_chunk_reference_cpu.py): the walk's table, header extent, line count, carry offset
and error triple; the staged sequences, byte for byte, with the zeros between and behind them; the gathered lines with *bytes
and *n_passed; a line carried into another chunk.  Equality is exact everywhere.  The shapes are the smallest at which the
kernels can go wrong: line and tab counts around a wave's 64 lanes, bytes around the 16 KiB slice of the byte index, more than
one slice of 2 048 lines, SEQ lengths and addresses around the 16-byte stores.  One context and one chunk serve the whole
module, reused across cases on purpose.  tests/test_gpu_sam_device.py checks the route as a whole against the host route."""
import ctypes as C
import types

import pytest

from tests import bamchunk as B
from tests import harness as H
from tests import samchunk as S

pytestmark = pytest.mark.gpu
SLICE = 16384                                                       # kChunkSliceBytes


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


NAMES = ("records", "n_header_lines", "header_end", "n_lines", "next", "error", "error_line", "error_off")


def check_walk(chunk, text, at_end, in_header, what=""):
    got, exp = chunk.sam_walk(at_end, in_header, cap=max(16, len(text) // 16 + 16)), S.ref_walk(text, at_end, in_header)
    for name, g, e in list(zip(NAMES, got, exp))[1:]:
        assert g == e, "%s (at_end %d, in_header %d): %s is %r, reference %r" % (what, at_end, in_header, name, g, e)
    assert len(got[0]) == len(exp[0]), "%s: %d records, reference %d" % (what, len(got[0]), len(exp[0]))
    for i, (g, e) in enumerate(zip(got[0], exp[0])):
        assert g == e, "%s: record %d is %r, reference %r" % (what, i, g, e)
    return got


def walk_all_ways(chunk, text, what):
    for at_end in (True, False):
        for in_header in (True, False):
            chunk.reset()
            check_walk(chunk, chunk.upload(text, 0), at_end, in_header, what)


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_walk_edge_cases(env, name):
    """Every well-formed case under both at_end values (the second leaves an unfinished last line as the carry) and both
    in_header values (behind the header, a leading '@' line is the error)."""
    walk_all_ways(env.chunk, S.edge_cases()[name], name)


@pytest.mark.parametrize("name", sorted(S.error_cases()))
def test_walk_error_cases(env, name):
    text, kind, line = S.error_cases()[name]
    env.chunk.reset()
    got = check_walk(env.chunk, env.chunk.upload(text, 0), True, True, name)
    assert got[5:7] == (kind, line)
    walk_all_ways(env.chunk, text, name)
    walk_all_ways(env.chunk, text.replace(b"\n", b"\r\n"), name + " (crlf)")


def short_lines(n, tabs_in_last=10):
    lines = [S.sam_line(b"q%d" % i, b"ACGT"[:1 + i % 4]) for i in range(n)]
    if n:
        lines[-1] = S.sam_line(b"last", b"AC", tags=(b"X:i:1",) * (tabs_in_last - 10))
    return b"".join(lines)


def test_walk_line_and_tab_counts_around_a_wave(env):
    """0, 1, 63, 64 and 65 lines; 63, 64 and 65 tabs in the whole chunk; with and without a header line in front."""
    chunk = env.chunk
    for text in (b"", b"no newline and no tab", b"\n"):
        walk_all_ways(chunk, text, "%r" % text)
    for n in (1, 63, 64, 65):
        walk_all_ways(chunk, short_lines(n), "%d lines" % n)
        walk_all_ways(chunk, b"@CO\tx\n" * (n - 1) + short_lines(1), "%d lines, one record" % n)
        walk_all_ways(chunk, b"@CO\n" * n, "%d header lines" % n)
    for tabs in (63, 64, 65):
        text = short_lines(6, tabs - 50)
        assert text.count(b"\t") == tabs
        walk_all_ways(chunk, text, "%d tabs" % tabs)
        # ... and one tab short in the last line: the chunk's last tab is the line's ninth
        cut = text[:text.rfind(b"\n")].rsplit(b"\t", tabs - 59)[0] + b"\n"
        assert cut.count(b"\t") == 59
        walk_all_ways(chunk, cut, "59 tabs, the last line has nine")


@pytest.mark.parametrize("at", [SLICE - 1, SLICE, SLICE + 1])
def test_walk_bytes_around_a_slice(env, at):
    """A line's first byte, a tab (the line's first; the one in front of SEQ; the one behind it) and a '\\n' at bytes 16 383,
    16 384 and 16 385: the last byte of a slice of the byte index, the first of the next, and the one behind it."""
    tail = S.sam_line(b"after", b"TTAGGG" * 4, tags=(b"NM:i:0",)) + S.sam_line(b"star", b"*", b"*") + S.sam_line(b"end", b"ACGT")
    pad = lambda n: b"@CO\t" + b"p" * (n - 5) + b"\n"               # noqa: E731  (a header line of n bytes)
    texts = {"line start": pad(at) + tail}
    rec = S.sam_line(b"N", b"ACGTACGT", tags=(b"RG:Z:x",))
    first_tab, seq_tab, qual_tab = 1, rec.index(b"\tACGTACGT\t"), rec.index(b"\tIIIIIIII")
    for what, where in (("first tab", first_tab), ("tab in front of SEQ", seq_tab), ("tab behind SEQ", qual_tab), ("newline", len(rec) - 1)):
        text = pad(at - where) + rec + tail
        assert text[at:at + 1] == rec[where:where + 1] and text[at - where - 1:at - where] == b"\n"
        texts[what] = text
    assert texts["line start"][at - 1:at + 1] == b"\na"
    for what, text in texts.items():
        walk_all_ways(env.chunk, text, "%s at %d" % (what, at))
        walk_all_ways(env.chunk, text.replace(b"\n", b"\r\n", 1).replace(b"pp", b"p", 1), "%s at %d, header crlf" % (what, at))


def test_walk_many_slices_of_lines(env):
    """More than two slices of 2 048 lines and more than a dozen slices of 16 KiB: the scans across waves, the header ending
    in the second slice of lines, a late error and a late header line, and a table that is too small."""
    header = b"".join(b"@SQ\tSN:c%d\tLN:%d\n" % (i, i) for i in range(2100))
    text = header + S.generated(8, 4000, 1, 40, header=b"")
    assert text.count(b"\n") > 3 * 2048 and len(text) > 12 * SLICE
    chunk = env.chunk
    chunk.reset()
    got = check_walk(chunk, chunk.upload(text, 0), True, True, "many slices")
    assert got[1] == 2100 and len(got[0]) > 4000
    chunk.reset()
    check_walk(chunk, chunk.upload(text[:-3], 0), False, True, "many slices, cut")
    recs = got[0]
    bad = bytearray(text)
    k = next(i for i in range(3000, len(recs)) if text[recs[i][0]:recs[i][0] + recs[i][3]].count(b"\t") == 10)
    bad[recs[k][0] + recs[k][1] - 1] = ord("x")                     # the tab in front of SEQ: nine tabs are left in the line
    bad[recs[3500][0]] = ord("@")
    chunk.reset()
    late = check_walk(chunk, chunk.upload(bytes(bad), 0), True, True, "late errors")
    assert k < 3500 and late[5:7] == (S.TOO_FEW_FIELDS, 2100 + k) and len(late[0]) == k
    bad[recs[k][0] + recs[k][1] - 1] = ord("\t")
    chunk.reset()
    late = check_walk(chunk, chunk.upload(bytes(bad), 0), True, True, "late header line")
    assert late[5:7] == (S.HEADER_AFTER_RECORD, 2100 + 3500)
    # cap < n: INVALID_ARG, *n says what is needed, the table's first entries are filled and nothing behind them
    chunk.reset()
    chunk.upload(text, 0)
    rc, arr, (n, headers, header_end, n_lines, nxt), _ = chunk.sam_walk_raw(True, True, 10)
    assert rc == env.K.TS_ERR_INVALID_ARG and n == len(recs) and (headers, header_end, nxt) == (2100, len(header), len(text))
    assert (arr[9].off, arr[9].size, arr[9].seq_len) == (recs[9][0], recs[9][3], recs[9][2])
    assert bytes(arr)[10 * C.sizeof(env.K.SamRecord):] == b"\xee" * C.sizeof(env.K.SamRecord)


def test_walk_chunked_with_carry(env):
    """A text in pieces: each piece goes behind what the walk before left unconsumed, the header state moves on as the route
    moves it, and the tables put together are the table of the whole text."""
    text = S.edge_cases()["generated crlf"]
    whole = S.ref_walk(text, True, True)
    for size in (37, 211, 4099):
        chunk = env.chunk
        chunk.reset()
        nxt, base, table, headers, lines, in_header = 0, 0, [], 0, 0, True
        pieces = [text[a:a + size] for a in range(0, len(text), size)]
        for k, piece in enumerate(pieces):
            held = chunk.upload(piece, nxt)
            base += nxt
            got = check_walk(chunk, held, k == len(pieces) - 1, in_header, "piece %d of %d bytes" % (k, size))
            table += [(r[0] + base,) + r[1:] for r in got[0]]
            headers, lines, nxt = headers + got[1], lines + got[3], got[4]
            in_header = in_header and got[1] == got[3]
        assert table == whole[0] and (headers, lines) == (whole[1], whole[3])


def stage_text():
    """SEQ of 1, 15, 16, 17 and 33 bases (and three lengths around the stage's 8 192-byte pieces), each at every address mod 16."""
    prefix = b"\t4\t*\t0\t0\t*\t*\t0\t0\t"
    lengths, out, at = [], [], 0
    for n in (1, 15, 16, 17, 33, 8191, 8192, 8209):
        for phase in range(16):
            name = b"n" * ((phase - at - len(prefix)) % 16 or 16)
            line = name + prefix + (b"TTAGGGA" * (n // 7 + 1))[:n] + b"\t*" + (b"\r\n" if phase % 5 == 2 else b"\n")
            assert (at + len(name) + len(prefix)) % 16 == phase
            out.append(line)
            lengths.append(n)
            at += len(line)
        out.append(S.sam_line(b"none", b"*", b"*"))
        at += len(out[-1])
    return b"".join(out), lengths


def test_stage_every_length_and_alignment(env):
    text, lengths = stage_text()
    chunk = env.chunk
    chunk.reset()
    recs = check_walk(chunk, chunk.upload(text, 0), True, True, "stage text")[0]
    with_seq = [r for r in recs if not r[4]]
    assert [r[2] for r in with_seq] == lengths and len(recs) == len(with_seq) + 8
    for n in set(lengths):
        assert {(r[0] + r[1]) % 16 for r in with_seq if r[2] == n} == set(range(16))
    reads = [S.ref_sequence(text, r) for r in with_seq]
    batch = B.ReadBatch(env.ctx, lengths)
    try:
        for _ in range(2):                                          # (the second time into a buffer that holds the first)
            assert chunk.sam_stage(with_seq, batch.ptr) == env.K.TS_OK, env.L.ts_last_error(env.ctx)
            assert all(o % 16 == 0 for o in batch.offsets)
            got, exp = batch.image(), batch.expected_image(reads)   # (every byte between and behind the reads is zero)
            assert len(got) == len(exp)
            if got != exp:
                at = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
                raise AssertionError("input buffer differs first at byte %d: %r, expected %r" % (at, got[at:at + 16], exp[at:at + 16]))
        # a record without sequence, or a segment of another length, is refused
        one = B.ReadBatch(env.ctx, [1])
        assert chunk.sam_stage([r for r in recs if r[4]][:1], one.ptr) == env.K.TS_ERR_INVALID_ARG
        assert chunk.sam_stage([r for r in with_seq if r[2] == 15][:1], one.ptr) == env.K.TS_ERR_INVALID_ARG
        one.close()
    finally:
        batch.close()


def test_gather_pass_vectors(env):
    """Lines of every size mod 16 (consecutive sizes, some with CR LF, the last without its newline), gathered under no, every
    and every other pass byte and two more patterns: the passing lines with a '\\n' behind each, in input order; then a
    host_out that is too small."""
    chunk = env.chunk
    lines = [S.sam_line(b"g", b"A" * (1 + i), b"*", eol=b"\r\n" if i % 6 == 1 else b"\n") for i in range(50)]
    text = S.HEADER + b"".join(lines) + S.sam_line(b"end", b"TTAGGG" * 300)[:-1]
    chunk.reset()
    recs = check_walk(chunk, chunk.upload(text, 0), True, True, "gather text")[0]
    n = len(recs)
    assert n == 51 and {r[3] % 16 for r in recs} == set(range(16)) and recs[-1][3] > 1800
    d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, n)
    assert d_pass
    vectors = [bytes(n), bytes([1]) * n, bytes(i % 2 for i in range(n)), bytes((i + 1) % 2 * 255 for i in range(n)),
               bytes(1 if i in (0, n - 1) else 0 for i in range(n))]
    for v in vectors:
        B.to_device(d_pass, v)
        exp, kept = S.ref_gather(text, recs, v)
        rc, out, nbytes, npassed = chunk.sam_gather(recs, d_pass, len(exp) + 64)
        assert rc == env.K.TS_OK, env.L.ts_last_error(env.ctx)
        assert (nbytes, npassed) == (len(exp), kept)
        assert out[:nbytes] == exp and out[nbytes:] == b"\xa5" * 64
    B.to_device(d_pass, vectors[1])
    exp, kept = S.ref_gather(text, recs, vectors[1])
    assert exp.endswith(b"\n") and not text.endswith(b"\n") and exp.count(b"\r\n") == 9
    rc, out, nbytes, npassed = chunk.sam_gather(recs, d_pass, len(exp) - 1)
    assert rc == env.K.TS_ERR_INVALID_ARG and (nbytes, npassed) == (len(exp), kept) and out == b"\xa5" * (len(exp) - 1)
    # a record that leaves the chunk is refused
    outside = [(recs[-1][0], recs[-1][1], recs[-1][2], recs[-1][3] + 1, 0)]
    assert chunk.sam_gather(outside, d_pass, 4096)[0] == env.K.TS_ERR_INVALID_ARG


def test_carry_into_another_chunk(env):
    """ts_chunk_carry_over: the unfinished line of one chunk goes to the front of another, the rest of the text behind it, and
    the walk of the joined line gives the rest of the whole text's table."""
    text = S.edge_cases()["generated"]
    whole = S.ref_walk(text, True, True)
    a, b = env.chunk, S.Chunk(env.ctx, 64, 256)
    try:
        for cut in (len(S.HEADER) - 7, len(text) // 2, len(text) // 2 + 33):
            a.reset()
            head = check_walk(a, a.upload(text[:cut], 0), False, True, "head")
            nxt = head[4]
            assert 0 < nxt < cut
            assert env.L.ts_chunk_carry_over(b.ptr, a.ptr, nxt, None) == env.K.TS_OK, env.L.ts_last_error(env.ctx)
            b.mirror = text[nxt:cut]
            assert b.size() == cut - nxt and b.read(0, cut - nxt) == text[nxt:cut]
            joined = b.upload(text[cut:], 0)
            rest = check_walk(b, joined, True, head[1] == head[3], "the joined line and what follows")
            assert head[0] + [(r[0] + nxt,) + r[1:] for r in rest[0]] == whole[0]
            assert head[1] + rest[1] == whole[1] and head[3] + rest[3] == whole[3] and rest[5] == S.OK
    finally:
        b.close()
