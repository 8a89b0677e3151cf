"""The deflate decoder core and CRC arithmetic of the BGZF kernel (teloscope_amd/csrc/inflate_core.h), compiled for the host by
g++ under ASan + UBSan (tests/cpp/inflate_core_host.cpp) and compared with zlib: clean blocks of every block type byte for
byte, damaged blocks verdict for verdict.  The kernel compiles the same functions, so a decoder that walks off a buffer is a
sanitizer report here and not a fault on a GPU.  No GPU needed.

What the decoder is fed: streams of zlib's own encoder (seven settings, five kinds of content, the sizes of SIZES), those
streams damaged (bit flips, truncations, a trailing byte), the members of the 512-file mutation suite, and the handmade
streams of tests/deflategen.py, which no encoder here emits: one match at every place of a batch and at every distance
around the 64 bytes written at a time, chains of matches that copy each other, batches of 64 longest matches, members of
up to eight blocks of all types in all orders, code-length sets that reach the decode paths behind the lookups, and one
broken table rule per member.  Third-party encoders (libdeflate, igzip, zopfli) are not among them."""
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflategen
from tests.test_bam_subset import bgzf, build_bam, make_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_DEFLATE, BAD_CRC = 0, 1, 2

# (name, level, strategy)
SETTINGS = [("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("l1", 1, zlib.Z_DEFAULT_STRATEGY),
            ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY), ("huffman", 6, zlib.Z_HUFFMAN_ONLY),
            ("rle", 6, zlib.Z_RLE)]
SIZES = [0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65280, 65536]


def deflate(data, level, strategy):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def zlib_verdict(payload, isize, crc):
    """What the host route's inflateBgzfBlock decides, by zlib alone: (class, bytes or None)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return BAD_DEFLATE, None
    if not d.eof or d.unused_data or len(out) != isize:
        return BAD_DEFLATE, None
    return (OK if zlib.crc32(out) & 0xFFFFFFFF == crc else BAD_CRC), out


def contents(rng):
    n = 65536
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)
    dna = (nib[rng.integers(0, 4, n)] << 4 | nib[rng.integers(0, 4, n)]).astype(np.uint8).tobytes()
    qual = np.clip(rng.normal(30, 8, n), 0, 60).astype(np.uint8).tobytes()
    one = b"\x47" * n
    block = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    far = block + block[:30000]                                    # distance 32 768, length 258
    header, records, _ = build_bam(make_reads(), 60000)
    stream = (header + b"".join(records))[:n]
    assert len(stream) == n
    return {"dna": dna, "qual": qual, "one": one, "far": far + dna[:n - len(far)], "bam": stream}, far


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_core")
    exe = str(d / "inflate_core_host")
    src = os.path.join(ROOT, "tests", "cpp", "inflate_core_host.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    empty = d / "empty.cases"
    empty.write_bytes(struct.pack("<I", 0))
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe, str(empty), str(d / "empty.out")], capture_output=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]

    def run(cases, tag):
        """cases: [(payload, isize, crc)] -> [(verdict, bytes)]; any sanitizer report fails the run."""
        fin, fout = d / (tag + ".cases"), d / (tag + ".out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for payload, isize, crc in cases:
                f.write(struct.pack("<III", len(payload), isize, crc) + payload)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, timeout=1200, env=env)
        assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
        raw = fout.read_bytes()
        out, at = [], 0
        for _ in cases:
            v, m = struct.unpack_from("<BI", raw, at)
            out.append((v, raw[at + 5:at + 5 + m]))
            at += 5 + m
        assert at == len(raw)
        return out
    return run


def test_clean_blocks_equal_zlib(host_decoder):
    rng = np.random.default_rng(2024)
    data, far = contents(rng)
    cases, want, btypes, multi, by_setting = [], [], set(), set(), {}
    for name, level, strategy in SETTINGS:
        pieces = [(k, v[:n]) for k, v in data.items() for n in SIZES] + [("far_exact", far)]
        for kind, plain in pieces:
            payload = deflate(plain, level, strategy)
            if len(payload) > 65536:                               # no BGZF member holds it (65 536 bytes stored, noise in fixed codes)
                assert len(plain) >= 65280, (name, kind, len(plain))
                continue
            first = payload[0]
            btypes.add((first >> 1) & 3)
            if not first & 1:
                multi.add(name)
            by_setting.setdefault(name, set()).add((first >> 1) & 3)
            cases.append((payload, len(plain), zlib.crc32(plain) & 0xFFFFFFFF))
            want.append((name, kind, plain))
    assert btypes == {0, 1, 2}
    for name, _, _ in SETTINGS:                                    # (zlib stores what does not compress, whatever the setting)
        assert {"stored": 0, "fixed": 1}.get(name, 2) in by_setting[name], (name, by_setting[name])
    assert {"stored", "l1"} <= multi, multi
    for name, level, strategy in (("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY)):
        assert not deflate(data["qual"][:65000], level, strategy)[0] & 1, name
    assert len(cases) >= 7 * 5 * 10
    got = host_decoder(cases, "clean")
    for (payload, isize, crc), (name, kind, plain), (v, out) in zip(cases, want, got):
        assert zlib_verdict(payload, isize, crc) == (OK, plain)
        assert v == OK, (name, kind, isize, v)
        assert out == plain, (name, kind, isize)


def damaged_cases():
    """[(tag, payload, isize, crc)]: per encoder setting 300 bit flips, 100 truncations and a trailing byte on a 60 000-byte
    block, and the undamaged control."""
    rng = np.random.default_rng(7)
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)
    dna = (nib[rng.integers(0, 4, 30000)] << 4 | nib[rng.integers(0, 4, 30000)]).astype(np.uint8).tobytes()
    qual = np.clip(rng.normal(30, 8, 30000), 0, 60).astype(np.uint8).tobytes()
    plain = dna + qual
    crc = zlib.crc32(plain) & 0xFFFFFFFF
    gen = random.Random(4242)
    out = []
    for name, level, strategy in (SETTINGS[0], SETTINGS[1], SETTINGS[3], SETTINGS[2]):
        payload = deflate(plain, level, strategy)
        assert len(payload) <= 65536
        out.append((name + ":control", payload, len(plain), crc))
        for i in range(300):
            m = bytearray(payload)
            m[gen.randrange(len(m))] ^= 1 << gen.randrange(8)
            out.append(("%s:flip%d" % (name, i), bytes(m), len(plain), crc))
        for i in range(100):
            out.append(("%s:cut%d" % (name, i), payload[:gen.randrange(len(payload))], len(plain), crc))
        out.append((name + ":trail", payload + b"\0", len(plain), crc))
    return out, plain


def test_damaged_blocks_get_zlibs_verdict(host_decoder):
    cases, plain = damaged_cases()
    want = [zlib_verdict(p, n, c) for _, p, n, c in cases]
    count = {k: sum(1 for v, _ in want if v == k) for k in (OK, BAD_DEFLATE, BAD_CRC)}
    print("zlib's classes over %d cases: ok %d, bad deflate %d, bad CRC %d" % (len(cases), count[OK], count[BAD_DEFLATE], count[BAD_CRC]))
    assert count[BAD_DEFLATE] >= 200 and count[BAD_CRC] >= 200
    for (tag, _, _, _), w in zip(cases, want):
        if tag.endswith(":control"):
            assert w == (OK, plain), tag
        if tag.endswith(":trail") or ":cut" in tag:
            assert w[0] == BAD_DEFLATE, tag
    got = host_decoder([(p, n, c) for _, p, n, c in cases], "damaged")
    wrong = [(tag, w[0], g[0]) for (tag, _, _, _), w, g in zip(cases, want, got) if w[0] != g[0]]
    assert not wrong, wrong[:20]
    for (tag, _, _, _), w, g in zip(cases, want, got):
        if w[0] != BAD_DEFLATE:
            assert g[1] == w[1], tag


def mutation_files_512():
    """The 512 files of tests/test_bam_subset.py::test_bam_mutation_suite_512, from the same seed."""
    gen = random.Random(20260)
    reads = [("record_%d" % i, ("TTAGGG" * (3 + i % 9)) if i % 3 else "ACGT" * (5 + i % 7)) for i in range(24)]
    header, records, _ = build_bam(reads, 60000)
    payload = header + b"".join(records)
    roff = len(header)
    good = bgzf(payload, 700)
    blocks = []
    pos = 0
    while pos < len(good):
        size = struct.unpack_from("<H", good, pos + 16)[0] + 1
        blocks.append(good[pos:pos + size]); pos += size
    files = []
    for index in range(512):
        mode = index % 11
        if mode == 0:
            data = bytes(gen.getrandbits(8) for _ in range(gen.randrange(0, 3000)))
        elif mode == 1:
            data = good[:gen.randrange(len(good) + 1)]
        elif mode == 2:
            data = bgzf(payload[:gen.randrange(len(payload) + 1)], 700)
        elif mode == 3:
            m = bytearray(good); m[gen.randrange(len(m))] ^= 1 << gen.randrange(8); data = bytes(m)
        elif mode == 4:
            m = bytearray(payload); m[gen.randrange(len(m))] ^= 1 << gen.randrange(8); data = bgzf(bytes(m), 700)
        elif mode == 5:
            m = bytearray(payload); struct.pack_into("<i", m, roff, gen.randrange(-64, 4096)); data = bgzf(bytes(m), 700)
        elif mode == 6:
            m = bytearray(payload); m[roff + 12] = gen.randrange(256); data = bgzf(bytes(m), 700)
        elif mode == 7:
            m = bytearray(payload); struct.pack_into("<H", m, roff + 16, gen.randrange(65536)); data = bgzf(bytes(m), 700)
        elif mode == 8:
            m = bytearray(payload); struct.pack_into("<i", m, roff + 20, gen.randrange(-8, 1 << 20)); data = bgzf(bytes(m), 700)
        elif mode == 9:
            m = bytearray(good); at = gen.randrange(18); m[at] = gen.randrange(256); data = bytes(m)
        else:
            bl = list(blocks)
            k = gen.randrange(len(bl))
            if gen.random() < 0.5: del bl[k]
            else: bl.insert(k, bl[k])
            data = b"".join(bl)
        files.append(data)
    return files


def bgzf_members(data):
    """(payload, isize, crc) of the BGZF blocks a front end would locate in data, up to the first thing that is not one."""
    out, pos = [], 0
    while pos + 18 <= len(data):
        if data[pos:pos + 3] != b"\x1f\x8b\x08" or data[pos + 3] != 4:
            break
        xlen = struct.unpack_from("<H", data, pos + 10)[0]
        if pos + 12 + xlen > len(data):
            break
        total, at = None, pos + 12
        while at + 4 <= pos + 12 + xlen:
            slen = struct.unpack_from("<H", data, at + 2)[0]
            if data[at:at + 2] == b"BC" and slen == 2 and at + 6 <= pos + 12 + xlen:
                total = struct.unpack_from("<H", data, at + 4)[0] + 1
            at += 4 + slen
        if total is None or total < 12 + xlen + 8 or pos + total > len(data):
            break
        crc, isize = struct.unpack_from("<II", data, pos + total - 8)
        if isize > 65536:
            break
        out.append((data[pos + 12 + xlen:pos + total - 8], isize, crc))
        pos += total
    return out


def test_mutation_suite_512_blocks(host_decoder):
    cases = [c for data in mutation_files_512() for c in bgzf_members(data)]
    assert len(cases) > 1500
    got = host_decoder(cases, "mut512")
    want = [zlib_verdict(*c) for c in cases]
    assert [g[0] for g in got] == [w[0] for w in want]
    assert {w[0] for w in want} == {OK, BAD_DEFLATE, BAD_CRC}
    for w, g in zip(want, got):
        if w[0] != BAD_DEFLATE:
            assert g[1] == w[1]


@pytest.mark.parametrize("name", deflategen.ACCEPTED + ("tables_bad", "crc_grid"))
def test_handmade_streams_get_zlibs_verdict(host_decoder, name):
    """Every list of tests/deflategen.py (which has asserted each member's class with zlib's decoder): zlib's verdict, and
    zlib's bytes where it accepts.  The fixture fails on any sanitizer output."""
    cases, plains = deflategen.cases(name), deflategen.plains(name)
    want = [zlib_verdict(p, n, c) for _, p, n, c in cases]
    if name == "tables_bad":
        assert sum(1 for w in want if w[0] == BAD_DEFLATE) >= 200
    else:
        assert all(w[0] == OK for w in want)
    got = host_decoder([(p, n, c) for _, p, n, c in cases], "handmade_" + name)
    wrong = [(tag, w[0], g[0]) for (tag, _, _, _), w, g in zip(cases, want, got) if w[0] != g[0]]
    assert not wrong, wrong[:20]
    for (tag, _, _, _), w, g in zip(cases, want, got):
        if w[0] == OK:
            assert g[1] == w[1] == plains[tag], tag


def test_crc_of_short_members(host_decoder):
    """Stored members of 0..130 bytes with the right CRC32 and with one bit of it wrong."""
    cases = deflategen.cases("crc_grid")
    assert [n for _, _, n, _ in cases] == list(range(131))
    wrong = [(p, n, c ^ (1 << (n % 32))) for _, p, n, c in cases]
    got = host_decoder([(p, n, c) for _, p, n, c in cases] + wrong, "crc_grid_wrong")
    assert [v for v, _ in got] == [OK] * 131 + [BAD_CRC] * 131
    assert [zlib_verdict(*c)[0] for c in wrong] == [BAD_CRC] * 131
