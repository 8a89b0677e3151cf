"""The block search and the span decoder of the plain-gzip kernels (teloscope_amd/csrc/gzip_core.h), compiled for the host by
g++ under ASan + UBSan (tests/cpp/gzip_core_host.cpp) and compared with zlib, whose Z_BLOCK walk lists every block boundary;
and the host side of the gzip source (include/teloscope_mi355x_gzip.hpp: member headers, trailers, zlib taking over at an
exact bit) against gzread (tests/cpp/gzip_feed_host.cpp, same sanitizers).  The kernels compile the same functions, so a
decoder that walks off a buffer is a sanitizer report here and not a fault on a GPU.  No GPU needed.

What was found about the probe (the candidate test of a deflate block start): on the nine inputs of this file — FASTQ-like
reads, a FASTA with 60-column lines and a GFA with long S lines, 1.2 MB each, at levels 1, 6 and 9 — it accepts, among all bit
offsets of the first 256 KB, exactly the starts of the non-final dynamic blocks: no false candidate and none missed, at
levels 1 and 9 as at level 6."""
import os
import random
import struct
import subprocess
import zlib

import pytest

from tests import deflategen as D
from tests import gziptexts as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP, FINAL, FULL, BAD, EDGE = range(5)
NEVER = 0xFFFFFFFF
PROBE_SIZE, SPAN_SIZE = 1_200_000, 300_000


def build(d, name, extra=()):
    exe = str(d / name)
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe, "-lz"]
    for more in ([], ["-static-libasan"]):                         # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + more + list(extra))
        r = subprocess.run([exe], capture_output=True)
        if r.returncode == 2 and b"usage" in r.stderr:
            break
    assert r.returncode == 2 and b"usage" in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    return exe


def run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(cmd, capture_output=True, timeout=1200, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    return r.stdout.decode()


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_core")
    exe = build(d, "gzip_core_host")

    class Core:
        def walk(self, stream):
            """[(bit, plain offset, final, type)] of every block start, and the stream's end as type 9"""
            (d / "s.bin").write_bytes(stream)
            run([exe, "walk", str(d / "s.bin"), str(d / "walk.txt")])
            return [tuple(int(x) for x in line.split()) for line in (d / "walk.txt").read_text().splitlines()]

        def probe(self, stream, ranges):
            (d / "s.bin").write_bytes(stream)
            args = [str(x) for r in ranges for x in r]
            run([exe, "probe", str(d / "s.bin"), str(d / "probe.txt")] + args)
            return [int(x) for x in (d / "probe.txt").read_text().split()]

        def spans(self, cases):
            """cases: [dict(stream, start, stop, stop0, cap, hist_len, hist)] -> [(end_bit, n_out, final, status, symbols, bytes)]"""
            with open(d / "span.cases", "wb") as f:
                f.write(struct.pack("<I", len(cases)))
                for c in cases:
                    hist = c.get("hist", b"")
                    assert len(hist) in (0, 32768)
                    f.write(struct.pack("<7I", len(c["stream"]), c["start"], c.get("stop", NEVER), c.get("stop0", NEVER), c["cap"],
                                        c["hist_len"], len(hist)) + c["stream"] + hist)
            run([exe, "span", str(d / "span.cases"), str(d / "span.out")])
            raw, at, out = (d / "span.out").read_bytes(), 0, []
            for c in cases:
                end_bit, n_out, final, status = struct.unpack_from("<4I", raw, at)
                at += 16
                sym = struct.unpack_from("<%dH" % n_out, raw, at)
                at += 2 * n_out
                data = None
                if c.get("hist"):
                    data = raw[at:at + n_out]
                    at += n_out
                out.append((end_bit, n_out, final, status, sym, data))
            assert at == len(raw)
            return out
    return Core()


def history_before(plain, off):
    """the 32 KiB in front of plain[off], zeros where the text has not begun"""
    h = plain[max(0, off - 32768):off]
    return b"\0" * (32768 - len(h)) + h


# ------------------------------------------------------------------------------------------------------------------ the probe
@pytest.mark.parametrize("level", G.LEVELS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_probe_accepts_exactly_the_dynamic_block_starts(core, kind, level):
    stream = G.raw_deflate(kind, PROBE_SIZE, level)
    blocks = core.walk(stream)
    assert blocks[-1][3] == 9 and blocks[-1][1] == PROBE_SIZE
    starts = [b for b, _, final, typ in blocks if final == 0 and typ == 2]
    assert len(starts) >= 8
    # every non-final dynamic block start of the whole stream is accepted ...
    assert core.probe(stream, [(b, b + 1) for b in starts]) == starts
    # ... and among all bit offsets of the first 256 KB nothing else is
    limit = min(8 * 256 * 1024, 8 * len(stream))
    assert core.probe(stream, [(0, limit)]) == [b for b in starts if b < limit]


def test_probe_refuses_what_is_not_a_dynamic_block(core):
    rng = random.Random(1)
    noise = bytes(rng.randrange(256) for _ in range(20000))
    assert core.probe(noise, [(0, 8 * len(noise))]) == []
    s = D.Stream()
    s.fixed_block([65] * 100, False)
    s.stored_block(b"x" * 100, False)
    final_at = s.nbits()
    tokens = D.soup(rng, 500)
    lit, dist = D.tables_for(tokens, rng)
    s.dynamic_block(tokens, lit, dist, True)                        # a final dynamic block: not a place to start a span
    assert core.probe(s.bytes(), [(0, 8 * len(s.bytes()))]) == []
    s2 = D.Stream()
    s2.dynamic_block(tokens, lit, dist, False)
    s2.fixed_block([], True)
    assert 0 in core.probe(s2.bytes(), [(0, 8)]) and final_at > 0
    assert core.probe(s2.bytes()[:20], [(0, 8)]) == []              # the header runs past the window's last byte


# ------------------------------------------------------------------------------------------------- span decode and resolve
@pytest.mark.parametrize("level", G.LEVELS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_span_decode_from_every_block_start_equals_zlib(core, kind, level):
    """From every true block start, with the true 32 KiB in front of it: the bytes to the end of the stream, and the bytes
    up to each later boundary when the decode is told to stop there (stop bit on the boundary, and one bit behind the
    boundary before it, which must give the same end)."""
    plain, stream = G.text(kind, SPAN_SIZE), G.raw_deflate(kind, SPAN_SIZE, level)
    blocks = core.walk(stream)
    starts, end_bit = blocks[:-1], blocks[-1][0]
    assert len(starts) >= 3
    cases, want = [], []
    for i, (b, off, _, _) in enumerate(starts):
        base = dict(stream=stream, start=b, cap=SPAN_SIZE - off, hist_len=min(off, 32768), hist=history_before(plain, off))
        cases.append(dict(base)); want.append((end_bit, SPAN_SIZE - off, FINAL))
        for j in range(i + 1, len(starts)):
            b2, off2 = starts[j][0], starts[j][1]
            cases.append(dict(base, stop=b2)); want.append((b2, off2 - off, STOP))
            cases.append(dict(base, stop=starts[j - 1][0] + 1)); want.append((b2, off2 - off, STOP))
        if i + 2 < len(starts):                                     # in two calls, as when a candidate is stepped over
            cases.append(dict(base, stop0=starts[i + 1][0] - 1, stop=starts[i + 2][0])); want.append((starts[i + 2][0], starts[i + 2][1] - off, STOP))
    got = core.spans(cases)
    for c, w, g in zip(cases, want, got):
        off = SPAN_SIZE - c["cap"]
        end = (g[0] + 7) // 8 * 8 if w[2] == FINAL else g[0]        # (zlib's walk gives the stream's end rounded up to a byte)
        assert (end, g[1], g[3]) == w, (c["start"], c.get("stop"), g[:4], w)
        assert g[5] == plain[off:off + w[1]], (c["start"], c.get("stop"))
        assert g[2] == (1 if w[2] == FINAL else 0)


def test_span_without_history_leaves_markers_that_resolve(core):
    """History unknown (hist_len 32768) at a block start in mid-stream: what reaches in front of the span comes out as markers,
    everything else as bytes, and resolve with the true history gives zlib's bytes."""
    plain, stream = G.text("fastq", SPAN_SIZE), G.raw_deflate("fastq", SPAN_SIZE, 6)
    blocks = core.walk(stream)
    b, off = blocks[2][0], blocks[2][1]
    hist = history_before(plain, off)
    (g,) = core.spans([dict(stream=stream, start=b, cap=SPAN_SIZE - off, hist_len=32768, hist=hist)])
    assert g[3] == FINAL and g[5] == plain[off:]
    markers = [s for s in g[4] if s & 0x8000]
    assert markers and all(hist[s & 0x7fff] == plain[off + i] for i, s in enumerate(g[4]) if s & 0x8000)
    assert all(s == plain[off + i] for i, s in enumerate(g[4]) if not s & 0x8000)


# --------------------------------------------------------------------------------------------------------- handmade streams
def one_block(tokens, kind, rng, last=True):
    s = D.Stream()
    if kind == "fixed":
        s.fixed_block(tokens, last)
    else:
        lit, dist = D.tables_for(tokens, rng)
        s.dynamic_block(tokens, lit, dist, last)
    return s.bytes()


@pytest.mark.parametrize("kind", ["fixed", "dynamic"])
def test_distance_to_the_edge_of_the_history(core, kind):
    """A match that reaches exactly the first byte of the 32 KiB in front of the span, and one that reaches one byte further.
    Deflate has no code for a distance of 32 769 (the codes end at 32 768), so "one further" is 32 768 with 32 767 bytes
    vouched for, and a match at the span's second symbol that 32 768 takes to the history's second byte."""
    rng = random.Random(7)
    hist = bytes(rng.randrange(256) for _ in range(32768))
    cases = []
    for dist, hist_len in ((32768, 32768), (32768, 32767), (32768, 0), (1, 0), (5, 4), (5, 5)):
        stream = one_block([(10, dist)], kind, rng)                # the span's first symbol reaches `dist` back
        cases.append(dict(stream=stream, start=0, cap=100, hist_len=hist_len, hist=hist))
    g = core.spans(cases)
    assert g[0][3] == FINAL and g[0][4] == tuple(0x8000 | i for i in range(10)) and g[0][5] == hist[:10]
    assert g[1][3] == BAD and g[1][1] == 0                          # 32 767 bytes vouched for: 32 768 is one too far
    assert g[2][3] == BAD
    assert g[3][3] == BAD                                           # a member's first span: a marker is an error, as in zlib
    assert g[4][3] == BAD
    assert g[5][3] == FINAL and g[5][5] == (hist[-5:] * 2)
    # one literal first: now 32 768 reaches the history's second byte, and with 32 767 bytes vouched for that is its first
    stream = one_block([90, (10, 32768), (3, 32768)], kind, rng)
    h, h2 = core.spans([dict(stream=stream, start=0, cap=100, hist_len=n, hist=hist) for n in (32768, 32767)])
    assert h[3] == FINAL and h[5] == b"Z" + hist[1:11] + hist[11:14] and h2[3] == FINAL and h2[4] == h[4]


@pytest.mark.parametrize("kind", ["fixed", "dynamic"])
def test_long_match_that_starts_in_the_history_and_overlaps_itself(core, kind):
    rng = random.Random(8)
    hist = bytes(rng.randrange(256) for _ in range(32768))
    for dist in (1, 2, 3, 7, 63, 64, 65, 100, 257):
        stream = one_block([(258, dist), 33, (258, 300)], kind, rng)
        (g,) = core.spans([dict(stream=stream, start=0, cap=1000, hist_len=32768, hist=hist)])
        want = D.expand([(258, dist), 33, (258, 300)], before=hist)
        assert g[3] == FINAL and g[5] == want, dist
        assert g[4][:258] == tuple(0x8000 | (32768 - dist + (j % dist)) for j in range(258)), dist     # markers copy as markers


def test_stored_and_fixed_blocks_inside_a_span(core):
    rng = random.Random(9)
    hist = bytes(rng.randrange(256) for _ in range(32768))
    s, before, bounds = D.Stream(), bytearray(hist), []
    for k in range(9):
        bounds.append((s.nbits(), len(before) - 32768))
        if k % 3 == 0:
            tokens = D.soup(rng, 700, before=min(len(before), 32000), near=0.5)        # (half the matches reach far back)
            lit, dist = D.tables_for(tokens, rng)
            s.dynamic_block(tokens, lit, dist, False)
            before += D.expand(tokens, before=bytes(before))
        elif k % 3 == 1:
            data = bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 300])))
            s.stored_block(data, False)
            before += data
        else:
            tokens = D.soup(rng, 300, before=min(len(before), 32000))
            s.fixed_block(tokens, k == 8)
            before += D.expand(tokens, before=bytes(before))
    stream, plain = s.bytes(), bytes(before[32768:])
    assert zlib.decompressobj(-15, zdict=hist).decompress(stream) == plain
    cases = [dict(stream=stream, start=b, cap=len(plain) - off, hist_len=32768, hist=history_before(hist + plain, 32768 + off))
             for b, off in bounds]
    cases += [dict(c, stop=bounds[5][0]) for c in cases[:5]]
    got = core.spans(cases)
    for (b, off), g in zip(bounds, got):
        assert g[3] == FINAL and g[5] == plain[off:], b
    for (b, off), g in zip(bounds[:5], got[len(bounds):]):
        assert (g[0], g[3]) == (bounds[5][0], STOP) and g[5] == plain[off:bounds[5][1]], b


def test_span_that_fills_its_capacity(core):
    rng = random.Random(10)
    first = D.soup(rng, 400)
    l1, d1 = D.tables_for(first, rng)
    for second in ([65] * 100, [65] * 98 + [(3, 1), 66], [70, (100, 1)]):
        n2 = len(D.expand(second, before=b"x"))
        s = D.Stream()
        s.dynamic_block(first, l1, d1, False)
        mid = s.nbits()
        s.fixed_block(second, True)
        stream, total = s.bytes(), 400 + n2
        exact, short = core.spans([dict(stream=stream, start=0, cap=total, hist_len=0), dict(stream=stream, start=0, cap=total - 1, hist_len=0)])
        assert exact[3] == FINAL and exact[1] == total              # to the byte
        # one symbol too many: the span reports the last boundary it reached and what it had there
        assert short[3] == FULL and (short[0], short[1]) == (mid, 400)
    s = D.Stream()
    s.stored_block(b"q" * 500, True)
    exact, short = core.spans([dict(stream=s.bytes(), start=0, cap=500, hist_len=0), dict(stream=s.bytes(), start=0, cap=499, hist_len=0)])
    assert (exact[3], exact[1]) == (FINAL, 500) and (short[3], short[1], short[0]) == (FULL, 0, 0)


def test_a_window_that_ends_inside_a_block_and_damaged_blocks(core):
    stream = G.raw_deflate("gfa", SPAN_SIZE, 6)
    blocks = core.walk(stream)
    b1 = blocks[1][0]
    cut = stream[:(blocks[2][0] // 8) - 100]                        # ends inside the second block
    (g,) = core.spans([dict(stream=cut, start=0, cap=SPAN_SIZE, hist_len=0)])
    assert (g[3], g[0], g[1]) == (EDGE, b1, blocks[1][1])
    rng = random.Random(12)
    cases = []
    for _ in range(300):                                            # bit flips anywhere: the decoder's bounds under the sanitizers
        bad = bytearray(stream)
        at = rng.randrange(8 * len(bad))
        bad[at // 8] ^= 1 << (at % 8)
        cases.append(dict(stream=bytes(bad[:rng.choice([len(bad), rng.randrange(1, len(bad))])]), start=rng.choice([0, b1, rng.randrange(8 * 1000)]),
                          cap=rng.choice([SPAN_SIZE, 5000]), hist_len=32768))
    for g in core.spans(cases):
        assert g[3] in (STOP, FINAL, FULL, BAD, EDGE)


# -------------------------------------------------------------- members, trailers and the hand-over to zlib, without a device
def file_classes():
    good = G.gzip_file("fastq", SPAN_SIZE, 6)
    flip = bytearray(good); flip[len(good) // 2] ^= 0x10
    crc = bytearray(good); crc[-6] ^= 1
    isize = bytearray(good); isize[-2] ^= 1
    second = G.gzip_file("gfa", 200_000, 9)
    named = b"\x1f\x8b\x08\x1e\0\0\0\0\0\xff" + b"\x03\x00abc" + b"name\0" + b"comment\0"
    named += (zlib.crc32(named) & 0xffff).to_bytes(2, "little") + good[10:]
    bad_hcrc = bytearray(named); bad_hcrc[12] ^= 1
    co = zlib.compressobj(0, zlib.DEFLATED, 31)
    level0 = co.compress(G.text("gfa", 200_000)) + co.flush()
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    empty = co.compress(b"") + co.flush()
    return {"good": good, "truncated": good[:len(good) // 2], "cut_in_trailer": good[:-3], "wrong_crc": bytes(crc),
            "wrong_isize": bytes(isize), "flipped_bit": bytes(flip), "trailing_garbage": good + b"trailing garbage" * 10,
            "two_members": good + second, "second_header_cut": good + second[:5], "header_fields": named,
            "header_crc_wrong": bytes(bad_hcrc), "empty_member_first": empty + good, "level0": level0,
            "unknown_method": b"\x1f\x8b\x07" + good[3:], "second_member_damaged": good + second[:3000] + b"\xff" * 50 + second[3050:]}


@pytest.fixture(scope="module")
def feed(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_feed")
    exe = build(d, "gzip_feed_host")

    def both(data, window, blocks):
        (d / "in.gz").write_bytes(data)
        ref = run([exe, "gzread", str(d / "in.gz"), str(d / "ref.out")]).split()
        got = run([exe, "reader", str(d / "in.gz"), str(d / "got.out"), str(window), str(blocks)]).split()
        return ref, (d / "ref.out").read_bytes(), got, (d / "got.out").read_bytes()
    return both


CLASSES = file_classes()


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_members_trailers_and_fallback_equal_gzread(feed, name):
    """Same verdict as gzread and, where it accepts, the same bytes (a truncated file: what zlib could still produce).  Without a
    device (zlib reads every member), and with a stand-in that verifies one to three blocks per window and then hands over, so
    that zlib takes over and hands back at many bit offsets."""
    handed = 0
    for window, blocks in ((1 << 20, 0), (50_000, 1), (20_000, 2), (200_000, 3), (7000, 1)):
        ref, ref_bytes, got, got_bytes = feed(CLASSES[name], window, blocks)
        assert got[0] == ref[0], (name, window, blocks)
        if ref[0] == "ok":
            assert got_bytes == ref_bytes, (name, window, blocks)
            assert int(got[1]) + int(got[2]) == len(ref_bytes)
            handed += int(got[3]) if int(got[1]) else 0
    if name == "good":
        assert handed >= 3                                          # device bytes and zlib bytes in one member, several times over


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_in_header_and_library():
    import ctypes as C

    import teloscope_amd  # noqa: F401
    from teloscope_amd import _capi
    names = ["ts_gzip_create", "ts_gzip_destroy", "ts_gzip_decode", "ts_gzip_take", "ts_gzip_read", "ts_gzip_history",
             "ts_gzip_note_fallback", "ts_gzip_stats"]
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    lib = C.CDLL(_capi.LIB_PATH)
    for n in names:
        assert n + "(" in hdr and hasattr(lib, n) and n in _capi.SYMBOLS, n
    assert lib.ts_abi_version() == 4
    assert "#define TELOSCAN_ABI_VERSION 4" in " ".join(hdr.split())
    assert C.sizeof(_capi.GzipResult) == 40
