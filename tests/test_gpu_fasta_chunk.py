"""The FASTA stages on a resident chunk, one by one through ctypes against the plain references of tests/fastachunk.py (pinned
without a device by tests/test_fasta_chunk_reference_cpu.py): the walk's table, names and carry offset; the joined bases, byte
for byte, with the zeros between records; the runs.  Equality is exact everywhere.  One context and one chunk serve the whole
module, reused across cases on purpose."""
import random
import types

import pytest

from tests import bamchunk as B
from tests import fastachunk as F
from tests import harness as H

pytestmark = pytest.mark.gpu

SLICE = 16384


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("x.fa -c TTAGGG")
    tel = ta.Teloscope(user_input(opts, device=0))
    chunk = F.Chunk(tel._ctx.ptr, 64, 1 << 16)
    yield types.SimpleNamespace(K=K, L=K.lib(), tel=tel, ctx=tel._ctx.ptr, chunk=chunk)
    chunk.close()
    tel.close()


def check_walk(chunk, text, at_end, what=""):
    exp = F.ref_walk(text, at_end)
    rc, recs, nxt, names, n, nb = chunk.fasta_walk(at_end, cap=len(exp[0]) + 4, names_cap=len(exp[2]) + 16)
    assert rc == chunk.K.TS_OK, chunk.L.ts_last_error(chunk.ctx)
    assert (n, nxt, nb) == (len(exp[0]), exp[1], len(exp[2])), "%s: (n, next, names_bytes) %r, reference %r" % (
        what, (n, nxt, nb), (len(exp[0]), exp[1], len(exp[2])))
    for i, (g, e) in enumerate(zip(recs, exp[0])):
        assert g == e, "%s: record %d is %r, reference %r" % (what, i, g, e)
    assert names == exp[2], "%s: names differ" % what
    return recs, nxt, names


def check_join(chunk, text, recs, at_end, what=""):
    """Join and runs of `recs` against the references; -> the joined image."""
    img, offsets = F.ref_join(text, recs, at_end)
    runs = F.ref_runs(text, recs, at_end)
    rc, ptr, offs, total, n_runs = chunk.fasta_join(recs, at_end)
    assert rc == chunk.K.TS_OK, chunk.L.ts_last_error(chunk.ctx)
    assert (offs, total, n_runs) == (offsets, len(img), len(runs)), "%s: offsets / total / runs" % what
    assert all(o % 16 == 0 for o in offs)
    got = B.device_bytes(ptr, total) if total else b""
    if got != img:
        at = next(i for i, (a, b) in enumerate(zip(got, img)) if a != b)
        raise AssertionError("%s: the joined bases differ first at byte %d of %d" % (what, at, total))
    assert chunk.fasta_bases(0, total) == img
    rc, got_runs, n = chunk.fasta_runs(len(runs) + 2)
    assert rc == chunk.K.TS_OK and n == len(runs)
    for i, (g, e) in enumerate(zip(got_runs, runs)):
        assert g == e, "%s: run %d is %r, reference %r" % (what, i, g, e)
    if runs:                                                    # the cap protocol: too small a table says what is needed
        rc, _, n = chunk.fasta_runs(len(runs) - 1)
        assert rc == chunk.K.TS_ERR_INVALID_ARG and n == len(runs)
    return img


def check_all(chunk, text, at_end, what=""):
    recs, nxt, names = check_walk(chunk, text, at_end, what)
    check_join(chunk, text, recs, at_end, what)
    return recs, nxt, names


@pytest.mark.parametrize("name", sorted(F.edge_cases()))
def test_edge_cases(env, name):
    text = F.edge_cases()[name]
    for at_end in (True, False):
        env.chunk.reset()
        check_all(env.chunk, env.chunk.upload(text, 0), at_end, "%s, at_end %d" % (name, at_end))


def test_walk_cap_protocol(env):
    text = F.edge_cases()["generated"]
    env.chunk.reset()
    env.chunk.upload(text, 0)
    exp = F.ref_walk(text, True)
    rc, _, _, _, n, nb = env.chunk.fasta_walk(True, cap=len(exp[0]) - 1, names_cap=len(exp[2]))
    assert rc == env.K.TS_ERR_INVALID_ARG and (n, nb) == (len(exp[0]), len(exp[2]))
    rc, _, _, _, n, nb = env.chunk.fasta_walk(True, cap=len(exp[0]), names_cap=len(exp[2]) - 1)
    assert rc == env.K.TS_ERR_INVALID_ARG and (n, nb) == (len(exp[0]), len(exp[2]))
    rc, recs, _, names, _, _ = env.chunk.fasta_walk(True, cap=len(exp[0]), names_cap=len(exp[2]))
    assert rc == env.K.TS_OK and recs == exp[0] and names == exp[2]
    # records that are not the chunk's are refused, not joined
    bad = list(recs)
    bad[3] = bad[3][:3] + (bad[3][3] + 1,) + bad[3][4:]
    assert env.chunk.fasta_join(bad, True)[0] == env.K.TS_ERR_INVALID_ARG
    bad[3] = (len(text) - 5, 100) + bad[3][2:]
    assert env.chunk.fasta_join(bad, True)[0] == env.K.TS_ERR_INVALID_ARG


def test_body_crosses_a_slice_at_every_phase(env):
    """A body that starts at every byte phase of a 16-byte row and crosses two slice ends, with an N-run over each of them and
    over the 1 KB a wave writes per step."""
    gen = random.Random(21)
    for phase in range(16):
        name = b"p" * (5 + phase)
        bases = bytearray(F.random_bases(gen, 40000, gaps=False))
        for at in (1024 - 7, 2048 - 1, SLICE - 40 - phase, 2 * SLICE - 3, 30000):
            bases[at:at + 90] = b"N" * 90
        text = F.record_text(name, bytes(bases), 80) + F.record_text(b"tail", b"NNACGTNN", 3)
        env.chunk.reset()
        check_all(env.chunk, env.chunk.upload(text, 0), True, "phase %d" % phase)


def test_many_lines_and_slices(env):
    """More than 2 048 lines in one record and more than 64 x 2 048 lines in a chunk: the scans across waves of lines."""
    gen = random.Random(22)
    parts = [F.record_text(b"thin", F.random_bases(gen, 3000), 1)]
    for i in range(70):
        parts.append(F.record_text(b"r%d" % i, F.random_bases(gen, 2000 + i), 1, b"\r\n" if i % 5 == 0 else b"\n"))
    text = b"".join(parts)
    assert text.count(b"\n") > 64 * 2048
    env.chunk.reset()
    check_all(env.chunk, env.chunk.upload(text, 0), True, "many lines")
    env.chunk.reset()
    check_all(env.chunk, env.chunk.upload(text, 0), False, "many lines, not at the end")


def test_record_starts_and_headers_at_slice_edges(env):
    """A record start on the first and on the last byte of a slice, and a header line that spans two slices."""
    gen = random.Random(23)
    first = F.record_text(b"a", F.random_bases(gen, 20000), 70)
    first = first[:SLICE - 1] + b"\n"                           # the next '>' is byte SLICE: the first of a slice
    second = F.record_text(b"b", F.random_bases(gen, 20000), 70)
    second = second[:SLICE - 2] + b"\n"                         # the next '>' is byte 2 SLICE - 1: the last of a slice
    third = b">" + b"long name " * 30 + b"\n" + F.fold(F.random_bases(gen, 16000), 80)
    third = third[:SLICE - 120] + b"\n"                         # the next header line spans the slice end
    fourth = b">" + b"spanning header " * 20 + b"\nNNNNACGTNN\n"
    text = first + second + third + fourth
    assert text[SLICE] == 62 and text[2 * SLICE - 1] == 62
    h = text.index(b">spanning")
    assert h < 3 * SLICE - 1 < h + 200
    env.chunk.reset()
    recs, _, names = check_all(env.chunk, env.chunk.upload(text, 0), True, "slice edges")
    assert [r[0] for r in recs] == [0, SLICE, 2 * SLICE - 1, h]


def cut_kinds(text, cuts):
    recs = F.ref_walk(text, True)[0]
    kinds = set()
    for c in cuts:
        if text[c:c + 1] == b">" and text[c - 1:c] == b"\n":
            kinds.add("before >")
        if text[c - 1:c] == b"\n":
            kinds.add("behind newline")
        for off, text_len, body_at, *_ in recs:
            if off < c < off + body_at:
                kinds.add("header")
            elif off + body_at < c < off + text_len and text[c - 1:c] != b"\n":
                kinds.add("body")
    return kinds


def feed(chunk, text, size):
    """The text in pieces of `size` bytes, each behind what the walk before left: every chunk walked, joined and searched for
    runs against the references on the chunk's own bytes; -> all records with offsets in the whole text, their names, bases."""
    chunk.reset()
    pieces = [text[a:a + size] for a in range(0, len(text), size)]
    nxt, base, table, names, bases = 0, 0, [], [], []
    for k, piece in enumerate(pieces):
        held = chunk.upload(piece, nxt)
        base += nxt
        at_end = k == len(pieces) - 1
        recs, nxt, nm = check_all(chunk, held, at_end, "piece %d of %d bytes" % (k, size))
        for r in recs:
            table.append((r[0] + base, r[1], r[2], r[3]))
            names.append(nm[r[4]:r[4] + r[5]])
            bases.append(F.ref_bases(held, r, at_end))
    assert nxt == len(chunk.mirror)
    return table, names, bases


@pytest.mark.parametrize("size", [37, 211, 1000, 4099, 16389])
@pytest.mark.parametrize("which", ["generated", "generated crlf"])
def test_chunked_with_carry(env, which, size):
    """The tables of the chunks, put together, are the table of the whole text, wherever a piece ends."""
    text = F.edge_cases()[which]
    if size == 37:
        assert {"header", "body", "behind newline", "before >"} <= cut_kinds(text, range(size, len(text), size))
    table, names, bases = feed(env.chunk, text, size)
    whole, _, whole_names = F.ref_walk(text, True)
    assert table == [r[:4] for r in whole]
    assert names == [whole_names[r[4]:r[4] + r[5]] for r in whole]
    assert bases == [F.ref_bases(text, r) for r in whole]


def test_chunk_grows_for_one_record(env):
    """A record larger than the chunk was made for: the walk answers n = 0, next = 0 until its end arrives, and the chunk has
    grown twice by then."""
    gen = random.Random(24)
    big = F.record_text(b"big", F.random_bases(gen, 300_000), 80)
    text = big + F.record_text(b"small", b"ACGTNNNN", 4)
    chunk = F.Chunk(env.ctx, 64, 1 << 16)
    try:
        nxt, grown = 0, 0
        for a in range(0, len(text), 100_000):
            piece = text[a:a + 100_000]
            before = chunk.size()
            held = chunk.upload(piece, nxt)
            at_end = a + 100_000 >= len(text)
            if not at_end:
                recs, nxt, _ = check_walk(chunk, held, False, "growing")
                assert recs == [] and nxt == 0
                grown += before > 0
            else:
                recs, nxt, _ = check_all(chunk, held, True, "grown")
                assert [r[3] for r in recs] == [300_000, 8] and held == text
        assert grown >= 2
    finally:
        chunk.close()


@pytest.mark.parametrize("mode", ["stored", "zlib"])
def test_bgzf_members_equal_plain_upload(env, mode):
    """The same text uploaded plain and inflated from BGZF members, in one chunk object, gives the same table, bases and runs."""
    text = F.edge_cases()["generated"] + F.edge_cases()["crlf"]
    big = F.Chunk(env.ctx, 1 << 20, 1 << 20)
    try:
        plain = check_all(big, big.upload(text, 0), True, "plain")
        held = big.fill_plain(text, len(big.mirror), member=7001, mode=mode)
        assert held == text
        assert check_all(big, held, True, mode) == plain
        big.reset()
        assert check_all(big, big.upload(text, 0), True, "plain again") == plain
    finally:
        big.close()
