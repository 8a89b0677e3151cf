"""The two device checks behind the assembly record filters, stage by stage through ctypes against the plain references of
tests/filtercheck.py (pinned without a device by tests/test_filter_check_reference_cpu.py): ts_gfa_chunk_check on a walked
chunk — line counts, the flagged lines in input order with their codes, the lines handed to the host — and
ts_fasta_chunk_strict on the records of a walk.  Equality is exact everywhere.  One context and one chunk serve the whole
module, reused across cases on purpose."""
import random
import types

import pytest

from tests import fastachunk as F
from tests import filtercheck as FC
from tests import gfachunk as G
from tests import harness as H

pytestmark = pytest.mark.gpu

SLICE = 16384
LINES = 2048


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("x.fa -c TTAGGG")
    tel = ta.Teloscope(user_input(opts, device=0))
    chunk = FC.Chunk(tel._ctx.ptr, 1 << 16, 1 << 20)
    yield types.SimpleNamespace(K=K, L=K.lib(), tel=tel, ctx=tel._ctx.ptr, chunk=chunk)
    chunk.close()
    tel.close()


def load(chunk, text):
    chunk.reset()
    return chunk.upload(text, 0)


def check(chunk, text, at_end, what=""):
    """The check of the chunk, which holds `text`, against the reference; -> (n_lines, flagged, next)."""
    n_lines, flagged, nxt = chunk.walk_and_check(text, at_end)
    want = FC.ref_gfa_check(text, at_end)
    assert n_lines == want[0], "%s: %d lines, reference %d" % (what, n_lines, want[0])
    assert flagged == want[1], "%s: flagged %r, reference %r" % (what, flagged[:5], want[1][:5])
    return n_lines, flagged, nxt


# ------------------------------------------------------------------------------------------------------------ ts_gfa_chunk_check
OFFENCES = [b"H\tVN:Z:2.0", b"Sx\tb", b"O\to1\ta+", b"W\tsm\t0\tc\t0\t4\t>a", b"C\ta\t+\tb\t+\t0\t2M", b"S\ta\t4\tACGT", b"X\tfoo", b"S\ta\tAC\rGT"]


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_one_offence_among_n_lines(env, n):
    """The only offence in the first line, on both sides of a lane boundary and in the last line, the last line with and without
    its line end; every code in turn."""
    good = [b"S\ts%d\tACGT" % i if i % 3 else b"L\ta\t+\tb\t-\t0M" if i % 2 else b"" for i in range(n)]
    assert FC.ref_gfa_check(FC.gfa_text(good), True) == (n, [])
    for k, bad in enumerate(OFFENCES):
        for at in sorted({0, 62, 63, 64, n - 1} & set(range(n))):
            lines = list(good)
            lines[at] = bad
            for last_eol in (True, False):
                for eol in (b"\n", b"\r\n"):
                    text = FC.gfa_text(lines, eol, last_eol)
                    n_lines, flagged, _ = check(env.chunk, load(env.chunk, text), True, "%d lines, %r in line %d" % (n, bad, at))
                    assert n_lines == n and len(flagged) == 1 and flagged[0][0] == at
                    assert flagged[0][3] == (FC.HOST_DECIDES if k == 7 else k + 1)
                    if not last_eol:                            # without at_end the unfinished last line is not counted, nor judged
                        n_lines, flagged, nxt = check(env.chunk, load(env.chunk, text), False, "open last line")
                        assert n_lines == n - 1 and nxt == len(text) - len(lines[-1]) and len(flagged) == (0 if at == n - 1 else 1)


def test_every_probe_line_and_the_lines_for_the_host(env):
    """Every probe line in one text, in four framings: the flagged table is the reference's, and the lines handed to the host
    are the lines with a '\\r' inside them, exactly."""
    lines = FC.gfa_probe_lines()
    for eol, last_eol in ((b"\n", True), (b"\r\n", True), (b"\n", False), (b"\r\n", False)):
        text = FC.gfa_text(lines, eol, last_eol)
        _, flagged, _ = check(env.chunk, load(env.chunk, text), True, "probe lines")
        inside = sum(1 for b, e in FC.gfa_lines(text, True) if b"\r" in text[b:e])
        assert sum(1 for f in flagged if f[3] == FC.HOST_DECIDES) == inside > 10
        assert {f[3] for f in flagged} == {1, 2, 3, 4, 5, 6, 7, FC.HOST_DECIDES}


@pytest.mark.parametrize("name", sorted(G.edge_cases()))
def test_edge_cases_of_the_walk(env, name):
    for text in (G.edge_cases()[name], G.crlf(G.edge_cases()[name])):
        for at_end in (True, False):
            check(env.chunk, load(env.chunk, text), at_end, "%s, at_end %d" % (name, at_end))


def test_line_slices_and_many_flagged(env):
    """2 048 x 2 + 3 lines, most of them flagged: the flagged table is written by three waves in input order."""
    gen = random.Random(21)
    pool = OFFENCES + [b"S\tn\tACGT", b"", b"# c", b"P\tp\tn+\t*"]
    lines = [pool[gen.randrange(len(pool))] for _ in range(2 * LINES + 3)]
    text = FC.gfa_text(lines)
    n_lines, flagged, _ = check(env.chunk, load(env.chunk, text), True, "line slices")
    assert n_lines == 2 * LINES + 3 and len(flagged) > LINES and [f[0] for f in flagged] == sorted(f[0] for f in flagged)
    rc, nl, got, nf = env.chunk.gfa_check(True, cap=len(flagged) - 1)   # too small a table: nothing copied, the count says what is needed
    assert rc == env.K.TS_ERR_INVALID_ARG and nf == len(flagged) and nl == n_lines and got == []
    rc, nl, got, nf = env.chunk.gfa_check(True, cap=len(flagged))
    assert rc == env.K.TS_OK and got == flagged
    rc, *_ = env.chunk.gfa_check(False, cap=len(flagged))              # not the at_end of the walk
    assert rc == env.K.TS_ERR_INVALID_ARG


def test_carriage_returns_and_tags_at_row_and_slice_ends(env):
    """A '\\r' on the last byte of a 16-byte row, of a 1 KB step and of a 16 KB slice and on the first of the next, followed by a
    line feed (a line end) or not (the host's line); and an H line of 3 000 tags whose VN:Z:2 is the last, across a slice end."""
    for at in (15, 16, 1023, 1024, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE):
        for follow in (b"\n", b"A\n", b"\r\n", b""):
            head = b"S\tn\t" + b"A" * (at - 4)
            text = head + b"\r" + follow + (b"S\tm\tAC\n" if follow else b"")
            assert text[at] == 13
            n_lines, flagged, _ = check(env.chunk, load(env.chunk, text), True, "cr at %d before %r" % (at, follow))
            assert [f[3] for f in flagged] == ([FC.HOST_DECIDES] if follow in (b"A\n", b"\r\n") else [])
    tags = b"".join(b"\txy:i:%d" % i for i in range(3000))
    for tail, code in ((b"\tVN:Z:2", [1]), (b"\tVN:Z:", []), (b"\tVN:Z:1\tVN:Z:2.0\r", [1]), (b"\tVN:Z:3", [])):
        text = b"#" * (SLICE - 9000) + b"\nH" + tags + tail + b"\nS\ta\tAC\n"
        assert text.index(b"\nH") < SLICE < len(text) - 20
        _, flagged, _ = check(env.chunk, load(env.chunk, text), True, "H line, tail %r" % tail)
        assert [f[3] for f in flagged] == code


def test_cut_at_every_byte_of_a_line(env):
    """A text cut into two chunks at every byte of a line: the first walked and checked without at_end, its unfinished line
    carried into a second chunk with the rest behind it.  The carried line is counted once, and the flagged lines with their
    line numbers running over both chunks are the one-chunk answer."""
    lines = [b"S\ta\tACGT", b"", b"O\tx", b"S\tb\t12\tAC\tLN:i:2", b"H\tfoo:Z:x\tVN:Z:2.0", b"# c", b"X\r", b"S\tc\tA\rC", b"L\ta\t+\tb\t+\t0M", b"W\tw"]
    text = FC.gfa_text(lines, b"\r\n", False)
    whole_n, whole = FC.ref_gfa_check(text, True)
    assert whole_n == len(lines) and len(whole) == 6
    a = text.index(b"S\tb\t12")
    second = FC.Chunk(env.ctx, 1 << 16, 64)
    try:
        for cut in range(a - 2, a + len(lines[3]) + 4):
            n1, f1, nxt = check(env.chunk, load(env.chunk, text[:cut]), False, "prefix of %d bytes" % cut)
            second.carry_over(env.chunk, nxt)
            held = second.upload(text[cut:], 0)
            assert held == text[nxt:]
            n2, f2, nxt2 = check(second, held, True, "rest behind %d bytes" % cut)
            assert n1 + n2 == whole_n and nxt + nxt2 == len(text)
            assert f1 + [(i + n1, off + nxt, ln, code, typ) for i, off, ln, code, typ in f2] == whole
    finally:
        second.close()


# ------------------------------------------------------------------------------------------------------------ ts_fasta_chunk_strict
def strict(chunk, text, at_end=True, what=""):
    rc, recs, nxt, names, n, nb = chunk.fasta_walk(at_end, cap=text.count(b">") + 1, names_cap=len(text) + 16)
    assert rc == chunk.K.TS_OK, chunk.L.ts_last_error(chunk.ctx)
    assert recs == F.ref_walk(text, at_end)[0]
    got = chunk.fasta_strict(recs)
    assert got == FC.ref_has_sequence(text, recs), "%s: %r, reference %r" % (what, got, FC.ref_has_sequence(text, recs))
    return recs, got, nxt


@pytest.mark.parametrize("n", [1, 64, 65])
def test_strict_bodies(env, n):
    """n records whose bodies go through every body of the list; one of them holds its single base behind 16 KB of blank lines,
    in a later slice than the body's start."""
    far = b"\n" * 7000 + b"\r\n" * 5000 + b"g\n"
    bodies = [b + (b"" if not b or b.endswith(b"\n") else b"\n") for b in FC.BODIES] + [far, b"\n" * (SLICE + 5)]
    assert all(b in bodies for b in (b"", b"\n\n", b"\r\n", b"\r\r\n"))
    for shift in range(len(bodies) if n == 1 else 3):
        text = b"".join(b">r%d d\n" % i + bodies[(i + shift * (1 if n == 1 else 7)) % len(bodies)] for i in range(n))
        recs, got, _ = strict(env.chunk, load(env.chunk, text), True, "%d records, shift %d" % (n, shift))
        assert len(recs) == n
        if n > 1:
            assert 0 in got and 1 in got
    text = b">far\n" + far + b">none\n" + b"\n" * (SLICE + 5) + b">last\n\r\r\n"
    recs, got, _ = strict(env.chunk, load(env.chunk, text), True, "a base in a later slice")
    assert got == [1, 0, 0] and recs[2][3] == 1                       # "\r\r\n": one base, no sequence
    assert recs[0][0] // SLICE != (recs[0][0] + recs[0][1] - 3) // SLICE
    assert env.chunk.fasta_strict([recs[2], recs[0]]) == [0, 1]       # any subset of the table, in any order
    assert env.chunk.fasta_strict([]) == []


def test_strict_edge_cases_of_the_walk(env):
    for name, text in sorted(F.edge_cases().items()):
        for at_end in (True, False):
            strict(env.chunk, load(env.chunk, text), at_end, "%s, at_end %d" % (name, at_end))


def test_strict_record_across_a_chunk_cut(env):
    """A record that spans the cut: open in the first chunk (not in its table), carried into the second and judged there."""
    text = b">a\n\n\r\n>b x\n\n\n\n\nT\n>c\n\r\n>d\nAC\n"
    b_at = text.index(b">b")
    second = FC.Chunk(env.ctx, 1 << 16, 64)
    try:
        for cut in range(b_at + 5, text.index(b">c") + 2):       # (from the end of b's header line on: before it, a is the open one)
            recs1, got1, nxt = strict(env.chunk, load(env.chunk, text[:cut]), False, "prefix of %d bytes" % cut)
            assert nxt == b_at and got1 == [0]
            second.carry_over(env.chunk, nxt)
            held = second.upload(text[cut:], 0)
            recs2, got2, _ = strict(second, held, True, "rest behind %d bytes" % cut)
            assert got1 + got2 == [0, 1, 0, 1]
    finally:
        second.close()
