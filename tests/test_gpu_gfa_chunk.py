"""The GFA stage on a resident chunk, through ctypes against the plain reference of tests/gfachunk.py (pinned without a device by
tests/test_gfa_chunk_reference_cpu.py): the segment table with every field span, the P / H line table, the gathered text, the
carry offset and the lowest foreign line; the carry of an unfinished line into another chunk; ts_terminal_ends on segments that
lie in the chunk.  Equality is exact everywhere.  One context and one chunk serve the whole module, reused across cases on
purpose."""
import ctypes as C
import random
import struct
import types

import numpy as np
import pytest

from tests import gfachunk as G
from tests import harness as H
from tests.test_bam_subset import bgzf_fancy

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
    chunk = G.Chunk(tel._ctx.ptr, 1 << 20, 1 << 16)
    yield types.SimpleNamespace(K=K, L=K.lib(), tel=tel, ctx=tel._ctx.ptr, chunk=chunk)
    chunk.close()
    tel.close()


def check_walk(chunk, text, at_end, what=""):
    """The walk of the chunk, which holds `text`, against the reference; -> (segments, lines, text, next, foreign)."""
    exp = G.ref_walk(text, at_end)
    rc, segs, lines, gathered, nxt, foreign, counts = chunk.gfa_walk(at_end, seg_cap=len(exp[0]) + 3, line_cap=len(exp[1]) + 3,
                                                                     text_cap=len(exp[2]) + 16)
    assert rc == chunk.K.TS_OK, chunk.L.ts_last_error(chunk.ctx)
    assert counts == (len(exp[0]), len(exp[1]), len(exp[2])), "%s: counts %r, reference %r" % (what, counts, (len(exp[0]), len(exp[1]), len(exp[2])))
    assert (nxt, foreign) == (exp[3], exp[4]), "%s: (next, foreign) %r, reference %r" % (what, (nxt, foreign), exp[3:])
    for i, (g, e) in enumerate(zip(segs, exp[0])):
        assert g == e, "%s: segment %d is %r, reference %r" % (what, i, g, e)
    for i, (g, e) in enumerate(zip(lines, exp[1])):
        assert g == e, "%s: line %d is %r, reference %r" % (what, i, g, e)
    assert gathered == exp[2], "%s: the gathered text differs" % what
    return segs, lines, gathered, nxt, foreign


def load(chunk, text):
    chunk.reset()
    return chunk.upload(text, 0)


@pytest.mark.parametrize("name", sorted(G.edge_cases()))
def test_edge_cases(env, name):
    for text in (G.edge_cases()[name], G.crlf(G.edge_cases()[name])):
        for at_end in (True, False):
            check_walk(env.chunk, load(env.chunk, text), at_end, "%s, at_end %d" % (name, at_end))


def s_line(start, tab2, tab3, gen, tail=b"\tLN:i:1\tx\ty\n"):
    """An S line that starts at byte `start` with its second tab at byte tab2 and its third at tab3."""
    name = bytes(gen.choice(b"abcdefgh") for _ in range(tab2 - start - 2))
    seq = bytes(gen.choice(b"ACGT") for _ in range(tab3 - tab2 - 1))
    return b"S\t" + name + b"\t" + seq + tail


@pytest.mark.parametrize("phase", range(16))
def test_tab_placement(env, phase):
    """A sequence that crosses two slice ends, the line starting at every byte phase of a 16-byte row; its tabs on the last byte
    of a slice and the first of the next, on a lane's bytes 15 and 16 (of a 16-byte row: its last, and the next lane's first) and
    at the end of a 1 KB step."""
    gen = random.Random(30 + phase)
    pre = b"" if phase == 0 else b"#" * (phase - 1) + b"\n"
    pairs = [(SLICE - 1, 2 * SLICE - 1), (SLICE, 2 * SLICE), (SLICE - 1, SLICE), (15 + 16 * 2, 2 * SLICE + 15), (16 + 16 * 2, 2 * SLICE + 16),
             (1023, 33 * 1024 - 1), (1024, 33 * 1024), (31, 2 * SLICE + 1023)]
    for tab2, tab3 in pairs:
        for tail in (b"\tLN:i:1\tx\ty\n", b"\n", b"\t" + b"A" * 2 * SLICE + b"\r\n"):
            line = s_line(phase, tab2, tab3, gen, tail)
            text = pre + line + b"S\tnext\tACGT\n"
            assert text[tab2] == 9 and (text[tab3] == 9 or tail == b"\n") and text[phase:phase + 2] == b"S\t"
            segs, *_ = check_walk(env.chunk, load(env.chunk, text), True, "phase %d, tabs at %d and %d" % (phase, tab2, tab3))
            assert segs[0][0] == phase and segs[0][5] + phase == tab2 + 1 and segs[0][6] == tab3 - tab2 - 1


def test_a_line_of_40000_tabs(env):
    """More tabs in one line than a slice has bytes of anything else: in an S line, a P line and a foreign line."""
    for head in (b"S\tn\tACGT", b"S\tn", b"P\tp\tn+", b"H", b"L"):
        text = b"S\tfirst\tAC\n" + head + b"\t" * 40000 + b"\nS\tlast\tACGT\tx\n"
        check_walk(env.chunk, load(env.chunk, text), True, "%r and 40000 tabs" % head)


@pytest.mark.parametrize("kinds", [b"SPHL#e", b"S", b"P", b"H", b"L"])
def test_line_slices(env, kinds):
    """2 048 x 2 + 3 short lines: every kind's count crosses the end of a slice of lines."""
    text = G.mixed_lines(41, 2 * LINES + 3, kinds)
    assert text.count(b"\n") == 2 * LINES + 3
    for at_end in (True, False):
        check_walk(env.chunk, load(env.chunk, text + b"S\topen\tAC"), at_end, "kinds %r, at_end %d" % (kinds, at_end))


def test_cap_protocol(env):
    text = G.path_graph(5, 60, 6)
    exp = G.ref_walk(text, True)
    want = (len(exp[0]), len(exp[1]), len(exp[2]))
    assert all(want)
    load(env.chunk, text)
    for k in range(3):
        caps = [w - (1 if i == k else 0) for i, w in enumerate(want)]
        rc, _, _, _, _, _, counts = env.chunk.gfa_walk(True, *caps)
        assert rc == env.K.TS_ERR_INVALID_ARG and counts == want, (k, rc, counts)
    rc, segs, lines, gathered, _, _, counts = env.chunk.gfa_walk(True, *want)
    assert rc == env.K.TS_OK and (segs, lines, gathered) == exp[:3]


def test_carry_into_another_chunk(env):
    """A text cut at every byte of a window around a line end: the prefix walked without at_end, its unfinished line carried into
    a second chunk, the rest appended behind it — the two chunks' tables together are the whole text's, and the first chunk's
    bytes stay as they were (carry_over reads them back)."""
    text = G.edge_cases()["paths before their segments"] + G.path_graph(6, 12, 3) + b"S\tlast\tACGT\r\nE\tx"
    whole = G.ref_walk(text, True)
    line_end = text.index(b"\n", len(text) // 2)
    second = G.Chunk(env.ctx, 1 << 16, 64)
    try:
        for k, cut in enumerate(range(line_end - 12, line_end + 13)):
            head = load(env.chunk, text[:cut])
            s1, l1, t1, nxt, f1 = check_walk(env.chunk, head, False, "prefix of %d bytes" % cut)
            assert nxt == text.rfind(b"\n", 0, cut) + 1
            second.carry_over(env.chunk, nxt)
            if k % 2 == 0:                                      # (the first carry grows the 64-byte chunk)
                held = second.upload(text[cut:], 0)
            else:
                assert env.L.ts_chunk_reserve(second.ptr, len(text)) == env.K.TS_OK
                held = second.fill_plain(text[cut:], 0, member=700, mode="zlib")
            assert held == text[nxt:]
            s2, l2, t2, nxt2, f2 = check_walk(second, held, True, "rest behind %d bytes" % cut)
            assert nxt + nxt2 == len(text)
            assert s1 + [(s[0] + nxt,) + s[1:9] + (s[9] + len(t1), s[10]) for s in s2] == whole[0]
            assert l1 + [(l[0] + nxt, l[1], l[2], l[3] + len(t1)) for l in l2] == whole[1]
            assert t1 + t2 == whole[2]
            assert (f1 if f1 is not None else (f2[0] + nxt, f2[1])) == whole[4]
    finally:
        second.close()


def members(data):
    """(compressed bytes, descriptors) of a BGZF file as B.Chunk.fill takes them."""
    descs, pos, dst = [], 0, 0
    while pos < len(data):
        flags, xlen = data[pos + 3], struct.unpack_from("<H", data, pos + 10)[0]
        extra, at, total = data[pos + 12:pos + 12 + xlen], 0, None
        while at < len(extra):
            ln = struct.unpack_from("<H", extra, at + 2)[0]
            if extra[at:at + 2] == b"BC":
                total = struct.unpack_from("<H", extra, at + 4)[0] + 1
            at += 4 + ln
        hdr = 12 + xlen
        for bit in (8, 16):
            if flags & bit:
                hdr = data.index(b"\0", pos + hdr) + 1 - pos
        hdr += 2 if flags & 2 else 0
        crc, isize = struct.unpack_from("<II", data, pos + total - 8)
        descs.append((pos + hdr, total - hdr - 8, isize, crc, dst))
        dst += isize
        pos += total
    return data, descs


def test_bgzf_members_equal_plain_upload(env):
    text = G.path_graph(8, 90, 9) + G.edge_cases()["gfa2 with and without tags"]
    plain = check_walk(env.chunk, load(env.chunk, text), True, "plain")
    env.chunk.reset()
    held = env.chunk.fill(text, members(bgzf_fancy(text, 1777, random.Random(5))), 0)
    assert held == text
    assert check_walk(env.chunk, held, True, "bgzf") == plain
    assert check_walk(env.chunk, load(env.chunk, text), True, "plain again") == plain


def test_ends_from_where_they_lie(env):
    """ts_terminal_ends on TS_INPUT_DEVICE segments that point into the chunk (unaligned addresses, lengths 0 and 1 among them)
    equals the same call on host copies of the bases."""
    K = env.K
    gen = random.Random(9)
    seqs = [b"", b"A", b"CCCTAA" * 200 + G.bases(gen, 5001) + b"TTAGGG" * 200, G.bases(gen, 777, "start"), b"C", G.bases(gen, 40000, "end"), G.bases(gen, 17)]
    text = b"H\tVN:Z:1.0\n" + b"".join(b"S\t%s\t%s%s\n" % (b"n" * (i + 1), s, b"\tLN:i:0" if i % 2 else b"") for i, s in enumerate(seqs))
    segs, *_ = check_walk(env.chunk, load(env.chunk, text), True, "ends")
    base = env.chunk.data()
    assert base and [s[6] for s in segs] == [len(s) for s in seqs]
    assert len({(base + s[0] + s[5]) % 16 for s in segs}) >= 4
    arr = (K.SegmentIn * len(segs))()
    for i, s in enumerate(segs):
        arr[i].seq, arr[i].len, arr[i].tips_only, arr[i].input_format = base + s[0] + s[5], s[6], 1, K.TS_INPUT_DEVICE
    ends = np.zeros((len(segs), 2), dtype=np.uint32)
    rc = env.L.ts_terminal_ends(env.ctx, arr, len(segs), ends.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == K.TS_OK, env.L.ts_last_error(env.ctx)
    want = env.tel.terminalEnds(seqs)
    assert np.array_equal(ends, want) and want.any()
    assert env.chunk.read(0, len(text)) == text
