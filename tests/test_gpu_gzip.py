"""ts_gzip_decode on the GPU against zlib.decompress: plain gzip members decoded by many waves (teloscope_amd/csrc/gzip.hip), the
object alone.  Clean files of three kinds of text at three levels, cut into spans smaller and larger than a deflate block and
into windows that keep their history from one call to the next: bytes, CRC and end bits, and — the test that fails without
the feature — statistics that say the device produced every byte and nothing was left to zlib.  The kernels compile the
decoder that tests/test_gzip_core_cpu.py runs on the host under sanitizers, so that file comes first in any job that runs
this one.  Odd files (a level-0 file, one letter a million times, noise, two members, damaged copies) go through the
object and the zlib fallback together in tests/test_gpu_gzip_feed.py.  None of these tests is meant to make the device fault."""
import ctypes as C
import zlib

import pytest

from tests import gziptexts as G

pytestmark = pytest.mark.gpu

SIZE = 1_200_000
WINDOW_END, FINAL_BLOCK, NO_CANDIDATE, SPAN_OVERFLOW, BAD_DEFLATE = range(5)
HISTORY_EMPTY, HISTORY_KEPT, HISTORY_GIVEN = range(3)


@pytest.fixture(scope="module")
def ctx():
    import teloscope_amd as ta
    from teloscope_amd.cli import parse_cli, user_input
    tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=0))
    yield tel._ctx.ptr
    del tel


def stats(ctx):
    from teloscope_amd import _capi as K
    out = (C.c_uint64 * 6)()
    assert K.lib().ts_gzip_stats(ctx, out) == 0
    return list(out)


def decode_member(ctx, deflate, span, window, first_history=(HISTORY_EMPTY, b"")):
    """A raw deflate stream through ts_gzip_decode, `window` compressed bytes at a time, each window beginning in the byte the
    one before ended in -> (bytes, [result per window]).  A window that holds no whole block (nothing verified, and nothing
    wrong) is tried again twice as large; any other window without progress ends the loop."""
    from teloscope_amd import _capi as K
    L = K.lib()
    gz = L.ts_gzip_create(ctx, span)
    assert gz
    try:
        out, results, bit, grow = bytearray(), [], 0, 1
        mode, hist = first_history
        while True:
            byte0 = bit // 8
            piece = deflate[byte0:byte0 + window * grow]
            res = K.GzipResult()
            rc = L.ts_gzip_decode(gz, piece, len(piece), bit % 8, mode, hist, len(hist), C.byref(res))
            assert rc == 0, rc
            buf = C.create_string_buffer(max(int(res.plain_bytes), 1))
            assert L.ts_gzip_read(gz, 0, res.plain_bytes, buf) == 0
            got = buf.raw[:res.plain_bytes]
            assert zlib.crc32(got) & 0xFFFFFFFF == res.crc32
            out += got
            results.append((8 * byte0 + res.end_bit, res.status, res.plain_bytes, res.spans_probed, res.spans_chained, res.spans_dropped))
            if 8 * byte0 + res.end_bit == bit and res.status in (WINDOW_END, NO_CANDIDATE) and byte0 + len(piece) < len(deflate):
                grow *= 2
                continue
            grow = 1
            if res.status != WINDOW_END or 8 * byte0 + res.end_bit == bit:
                break
            bit = 8 * byte0 + res.end_bit
            mode, hist = HISTORY_KEPT, b""
        hbuf, hlen = C.create_string_buffer(32768), C.c_uint64(0)
        assert L.ts_gzip_history(gz, hbuf, C.byref(hlen)) == 0
        assert hbuf.raw[:hlen.value] == bytes(out[-32768:])[-hlen.value:] and hlen.value == min(32768, len(out))
        return bytes(out), results
    finally:
        L.ts_gzip_destroy(gz)


@pytest.mark.parametrize("window", [1 << 28, 100_000])
@pytest.mark.parametrize("span", [4096, 16384, 65536])
@pytest.mark.parametrize("level", G.LEVELS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_clean_text_is_decoded_by_the_device_alone(ctx, kind, level, span, window):
    plain, deflate = G.text(kind, SIZE), G.raw_deflate(kind, SIZE, level)
    before = stats(ctx)
    got, results = decode_member(ctx, deflate + b"\0" * 8, span, window)       # (a trailer's worth of bytes behind the stream)
    after = stats(ctx)
    print(kind, level, span, window, len(deflate), results[-3:], [a - b for a, b in zip(after, before)])
    assert got == plain
    end_bit, status = results[-1][:2]
    assert status == FINAL_BLOCK and (end_bit + 7) // 8 == len(deflate)
    windows, probed, chained, dropped, produced, to_zlib = [a - b for a, b in zip(after, before)]
    # tests/test_gzip_core_cpu.py shows the probe exact for these nine inputs: the device alone produces every byte
    assert to_zlib == 0 and produced == len(plain) and windows == len(results)
    assert chained == sum(r[4] for r in results) and probed == sum(r[3] for r in results)
    if window >= len(deflate) and span <= 16384:
        assert chained >= 8                                         # (many waves, not one)


def test_history_given_by_the_caller(ctx):
    """A decode that begins at a block boundary in mid-stream with the 32 KiB in front of it handed over, as after a stretch of
    zlib: the rest of the member comes out right."""
    plain, deflate = G.text("fastq", SIZE), G.raw_deflate("fastq", SIZE, 6)
    whole, results = decode_member(ctx, deflate + b"\0" * 8, 16384, 200_000)
    assert whole == plain and len(results) >= 2
    bit, done = results[0][0], results[0][2]
    tail = deflate[bit // 8:] + b"\0" * 8
    got, _ = decode_member_from(ctx, tail, bit % 8, 16384, plain[max(0, done - 32768):done])
    assert got == plain[done:]


def decode_member_from(ctx, deflate, start_bit, span, history):
    from teloscope_amd import _capi as K
    L = K.lib()
    gz = L.ts_gzip_create(ctx, span)
    assert gz
    try:
        res = K.GzipResult()
        assert L.ts_gzip_decode(gz, deflate, len(deflate), start_bit, HISTORY_GIVEN, history, len(history), C.byref(res)) == 0
        buf = C.create_string_buffer(max(int(res.plain_bytes), 1))
        assert L.ts_gzip_read(gz, 0, res.plain_bytes, buf) == 0
        assert res.status == FINAL_BLOCK
        return buf.raw[:res.plain_bytes], res
    finally:
        L.ts_gzip_destroy(gz)


def test_arguments_are_checked(ctx):
    from teloscope_amd import _capi as K
    L = K.lib()
    assert not L.ts_gzip_create(ctx, 1000) and not L.ts_gzip_create(ctx, 2 << 20)
    gz = L.ts_gzip_create(ctx, 4096)
    try:
        res = K.GzipResult()
        data = G.raw_deflate("gfa", SIZE, 6)
        assert L.ts_gzip_decode(gz, data, 0, 0, HISTORY_EMPTY, None, 0, C.byref(res)) == K.TS_ERR_INVALID_ARG
        assert L.ts_gzip_decode(gz, data, len(data), 8 * 4096, HISTORY_EMPTY, None, 0, C.byref(res)) == K.TS_ERR_INVALID_ARG
        assert L.ts_gzip_decode(gz, data, len(data), 0, 3, None, 0, C.byref(res)) == K.TS_ERR_INVALID_ARG
        assert L.ts_gzip_decode(gz, data, len(data), 0, HISTORY_GIVEN, None, 5, C.byref(res)) == K.TS_ERR_INVALID_ARG
        assert L.ts_gzip_read(gz, 0, 1, C.create_string_buffer(1)) == K.TS_ERR_INVALID_ARG
    finally:
        L.ts_gzip_destroy(gz)
