"""The deflate encoder core and its CRC32 (teloscope_amd/csrc/deflate_core.h), compiled for the host by g++ under ASan + UBSan
(tests/cpp/deflate_core_host.cpp) and judged by zlib: every payload inflates to its block, ends where the payload ends and is at
most five bytes longer than the block.  The kernel compiles the same functions, so an encoder that walks off a buffer is a
sanitizer report here and not a fault on a GPU.  The project's own decoder (tests/cpp/inflate_core_host.cpp) reads every payload
too.  No GPU needed; tests/test_gpu_bgzf_deflate.py holds the device against this program byte for byte."""
import zlib

import numpy as np
import pytest

from tests import deflatecases
from tests.deflatecases import MAX_BLOCK, dynamic_header, kraft, raw_inflate
from tests.test_inflate_core_cpu import host_decoder  # noqa: F401  (the fixture that builds the decoder's host program)

OK = 0


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    return deflatecases.build_host_encoder(tmp_path_factory.mktemp("deflate_core"), sanitize=True)


@pytest.fixture(scope="module")
def encoded(host_encoder):
    """{name: (plain, payload, crc)} of every block of deflatecases.named_blocks(), encoded once."""
    blocks = deflatecases.named_blocks()
    got = host_encoder([plain for _, plain in blocks], "all")
    return {name: (plain, payload, crc) for (name, plain), (payload, crc) in zip(blocks, got)}


def btype(payload):
    return (payload[0] >> 1) & 3


def test_every_block_round_trips(encoded, host_decoder):  # noqa: F811
    assert len(encoded) >= 6 * len(deflatecases.SIZES)
    kinds = set()
    for name, (plain, payload, crc) in encoded.items():
        assert raw_inflate(payload) == plain, name
        assert len(payload) <= len(plain) + 5, name
        assert crc == zlib.crc32(plain) & 0xFFFFFFFF, name
        assert payload[0] & 1, name                                 # one final block
        kinds.add(btype(payload))
    assert kinds == {0, 2}
    names = list(encoded)
    got = host_decoder([(encoded[k][1], len(encoded[k][0]), encoded[k][2]) for k in names], "deflated")
    for name, (verdict, out) in zip(names, got):
        assert verdict == OK and out == encoded[name][0], name


def test_empty_block_is_a_valid_final_block(encoded):
    plain, payload, crc = encoded["dna:0"]
    assert plain == b"" and payload == b"\x01\x00\x00\xff\xff" and crc == 0


def test_distance_limit(encoded):
    plain, payload, _ = encoded["far_exact"]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    level6 = len(co.compress(plain) + co.flush())
    print("far_exact: %d plain, %d payload, zlib level 6 %d" % (len(plain), len(payload), level6))
    # (zlib itself does not find this repeat: its window reaches 32 768 - 262 back, and level 6 measures 62 788 here)
    assert level6 > 60000
    assert len(payload) < 40000                                     # the repeat at exactly 32 768 is found: 30 000 bytes saved
    plain, payload, _ = encoded["far_plus1"]                        # 32 769 back: out of reach (and still round-trips, above)
    assert len(payload) > 62000
    assert raw_inflate(payload) == plain
    for lead in (1, 3, 4, 5, 64, 258):
        plain, payload, _ = encoded["front:%d" % lead]
        assert raw_inflate(payload) == plain


def test_matches_are_used(encoded):
    plain, payload, _ = encoded["one:65280"]
    assert len(plain) == MAX_BLOCK
    print("65 280 equal bytes: payload %d" % len(payload))
    assert len(payload) < MAX_BLOCK // 8
    plain, payload, _ = encoded["chain"]
    assert len(payload) < len(plain) // 8


def test_dynamic_codes_are_used(encoded):
    for kind in ("dna", "qual"):
        plain, payload, _ = encoded["%s:65280" % kind]
        print("%s: payload %d of %d" % (kind, len(payload), len(plain)))
        assert btype(payload) == 2
        assert len(payload) < len(plain)


def check_header(payload, name):
    clen, llen, dlen = dynamic_header(payload)
    assert max(clen) <= 7 and max(llen) <= 15 and max(dlen) <= 15, name
    assert llen[256] != 0, name
    assert kraft(clen) == 1 << 15 and kraft(llen) == 1 << 15, name
    assert kraft(dlen) == 1 << 15, name                             # (two one-bit codes where no or one distance is used)
    return clen, llen, dlen


def test_every_dynamic_header_is_one_zlib_accepts(encoded):
    seen = 0
    for name, (_, payload, _) in encoded.items():
        if btype(payload) == 2:
            check_header(payload, name)
            seen += 1
    assert seen > 50


def test_length_limit(encoded, host_encoder):
    plain, payload, _ = encoded["fibonacci"]
    assert btype(payload) == 2 and raw_inflate(payload) == plain
    check_header(payload, "fibonacci")
    # the length builder alone, on counts no block needs to be arranged for: Fibonacci counts are the deepest trees there are
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    cases = [(15, fib[:22] + [0] * 264), (15, [0] * 100 + fib[:24][::-1] + [0] * 162), (15, fib[:24] + [0] * 6),
             (7, fib[:19]), (7, fib[:12] + [0] * 7), (7, [0, 3, 0, 0, 0] + fib[:14]),
             (15, [1] * 286), (7, [1] * 19), (15, [0] * 286), (15, [0] * 30), (15, [0] * 7 + [5] + [0] * 22),
             (15, [9] + [0] * 29), (7, [0] * 18 + [4]), (15, [65280] + [1] * 285)]
    got = host_encoder.lengths(cases, "lengths")
    for (limit, counts), lens in zip(cases, got):
        lens = list(lens)
        assert max(lens) <= limit, (limit, counts)
        assert kraft(lens) == 1 << 15, (limit, counts, lens)
        assert all(l > 0 for l, c in zip(lens, counts) if c), (limit, counts, lens)
        assert sum(1 for l in lens if l) == max(2, sum(1 for c in counts if c)), (limit, counts, lens)
    # where the limit does not bind, the lengths are Huffman's own
    assert sorted(l for l in got[6] if l) == [8] * 226 + [9] * 60
    assert sorted(l for l in got[7] if l) == [4] * 13 + [5] * 6


def test_degenerate_alphabets(encoded):
    for name in ("one:1", "one:2", "two_bytes", "two_bytes_apart", "chain", "one:63", "one:64"):
        plain, payload, _ = encoded[name]
        assert raw_inflate(payload) == plain, name
    assert btype(encoded["one:63"][1]) == 2                         # one byte and the end-of-block symbol, no distance
    _, llen, dlen = check_header(encoded["one:63"][1], "one:63")
    assert sum(1 for l in llen if l) == 2 and [l for l in dlen if l] == [1, 1]
    assert btype(encoded["two_bytes"][1]) == 2
    for n in (1, 2, 63, 65280):                                     # noise has no match and no short code: stored
        plain, payload, _ = encoded["noise:%d" % n]
        assert btype(payload) == 0 and len(payload) == n + 5, n


def test_encoder_is_deterministic(encoded, host_encoder):
    names = [k for k in encoded if k.endswith(":65280") or k.endswith(":129")]
    again = host_encoder([encoded[k][0] for k in names][::-1], "again")[::-1]
    for name, (payload, crc) in zip(names, again):
        assert payload == encoded[name][1] and crc == encoded[name][2], name
