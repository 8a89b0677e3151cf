"""ts_bgzf_deflate on the GPU: the blocks of tests/deflatecases.py (every content at every edge size, the distance-limit,
length-limit and degenerate blocks), concatenated and cut into payloads of 1, 700 and 65 280 bytes, and each block alone.  Every
member is parsed here and judged by zlib; at 65 280 and for the single blocks every payload is held byte for byte against the
host build of the same encoder (tests/cpp/deflate_core_host.cpp, which tests/test_deflate_core_cpu.py runs under sanitizers on
these blocks, so that file comes first in any job that runs this one); ts_bgzf_inflate reads the members back."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import deflatecases
from tests.deflatecases import MAX_BLOCK

pytestmark = pytest.mark.gpu

HEAD = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0])


@pytest.fixture(scope="module")
def ctx():
    import teloscope_amd as ta
    from teloscope_amd.cli import parse_cli, user_input
    tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=0))
    yield tel._ctx.ptr
    del tel


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    return deflatecases.build_host_encoder(tmp_path_factory.mktemp("deflate_core_gpu"), sanitize=False)


@pytest.fixture(scope="module")
def blocks():
    return deflatecases.named_blocks()


@pytest.fixture(scope="module")
def whole(blocks):
    return b"".join(plain for _, plain in blocks)


def members_of(data):
    """[(payload, crc, isize)] of a run of BGZF members that must fill data exactly; header, BSIZE and size limit checked."""
    out, pos = [], 0
    while pos < len(data):
        assert data[pos:pos + 16] == HEAD, pos
        total = struct.unpack_from("<H", data, pos + 16)[0] + 1
        assert 26 < total <= 65536 and pos + total <= len(data), (pos, total)
        crc, isize = struct.unpack_from("<II", data, pos + total - 8)
        out.append((data[pos + 18:pos + total - 8], crc, isize))
        pos += total
    return out


def check_members(members, plain, payload_bytes):
    assert len(members) == -(-len(plain) // payload_bytes)
    for i, (payload, crc, isize) in enumerate(members):
        want = plain[i * payload_bytes:(i + 1) * payload_bytes]
        assert isize == len(want) and crc == zlib.crc32(want) & 0xFFFFFFFF, i
        assert len(payload) <= len(want) + 5, i
        assert deflatecases.raw_inflate(payload) == want, i


def stats(ctx):
    from teloscope_amd import _capi as K
    out = (C.c_uint64 * 4)()
    assert K.lib().ts_bgzf_deflate_stats(ctx, out) == K.TS_OK
    return list(out)


def inflate_back(ctx, data, members):
    from teloscope_amd import _capi as K
    from teloscope_amd.bgzf import inflate_blocks
    descr, src, dst = [], 0, 0
    for payload, crc, isize in members:
        descr.append((src + 18, len(payload), isize, crc, dst))
        src += 18 + len(payload) + 8
        dst += isize
    plain, (code, bad) = inflate_blocks(ctx, data, descr, dst)
    assert (code, bad) == (K.BGZF_OK, len(members))
    return plain


def test_payload_65280_equals_the_host_program(ctx, whole, host_encoder):
    from teloscope_amd.bgzf import deflate_blocks
    before = stats(ctx)
    data = deflate_blocks(ctx, whole, MAX_BLOCK)
    after = stats(ctx)
    members = members_of(data)
    check_members(members, whole, MAX_BLOCK)
    assert [a - b for a, b in zip(after, before)] == [1, len(members), len(whole), len(data)]
    cuts = [whole[i:i + MAX_BLOCK] for i in range(0, len(whole), MAX_BLOCK)]
    host = host_encoder(cuts, "cuts")
    assert {(p[0] >> 1) & 3 for p, _ in host} == {0, 2}
    for i, ((payload, crc, _), (hp, hc)) in enumerate(zip(members, host)):
        assert payload == hp and crc == hc, i
    assert inflate_back(ctx, data, members) == whole


def test_each_block_alone_equals_the_host_program(ctx, blocks, host_encoder):
    from teloscope_amd.bgzf import deflate_blocks
    host = host_encoder([plain for _, plain in blocks], "alone")
    for (name, plain), (hp, hc) in zip(blocks, host):
        data = deflate_blocks(ctx, plain, MAX_BLOCK)
        if not plain:
            assert data == b"", name                                # n = 0: no member
            continue
        members = members_of(data)
        assert len(members) == 1, name
        assert members[0] == (hp, hc, len(plain)), name
        assert deflatecases.raw_inflate(members[0][0]) == plain, name


def test_payload_700_more_members_than_resident_waves(ctx, whole):
    from teloscope_amd.bgzf import deflate_blocks
    data = deflate_blocks(ctx, whole, 700)
    members = members_of(data)
    assert len(members) >= 2000
    check_members(members, whole, 700)
    assert inflate_back(ctx, data, members) == whole


def test_payload_1(ctx, whole):
    """A member per byte: each is the stored form, 32 bytes, so the whole output is compared as one array."""
    from teloscope_amd.bgzf import deflate_blocks
    data = np.frombuffer(deflate_blocks(ctx, whole, 1), dtype=np.uint8)
    src = np.frombuffer(whole, dtype=np.uint8)
    assert len(data) == 32 * len(src)
    crc = np.array([zlib.crc32(bytes([b])) & 0xFFFFFFFF for b in range(256)], dtype="<u4")
    want = np.zeros((len(src), 32), dtype=np.uint8)
    want[:, :16] = np.frombuffer(HEAD, dtype=np.uint8)
    want[:, 16] = 31
    want[:, 18:23] = np.frombuffer(b"\x01\x01\x00\xfe\xff", dtype=np.uint8)
    want[:, 23] = src
    want[:, 24:28] = crc[src].view(np.uint8).reshape(-1, 4)
    want[:, 28] = 1
    assert np.array_equal(data.reshape(-1, 32), want)
    sample = members_of(data[:32 * 300].tobytes())
    check_members(sample, whole[:300], 1)


def test_cap_protocol_and_arguments(ctx, whole):
    from teloscope_amd import _capi as K
    L = K.lib()
    plain = whole[:200000]
    src = np.frombuffer(plain, dtype=np.uint8)
    nbytes, count = C.c_uint64(0), C.c_uint64(0)
    out = np.full(len(plain) + 1000, 0x5A, dtype=np.uint8)

    def call(payload_bytes, cap, n=len(plain)):
        return L.ts_bgzf_deflate(ctx, src.ctypes.data, n, payload_bytes, out.ctypes.data if cap else None, cap, C.byref(nbytes),
                                 C.byref(count))
    assert call(MAX_BLOCK, len(out)) == K.TS_OK
    need, members = nbytes.value, count.value
    assert members == -(-len(plain) // MAX_BLOCK) and 0 < need <= len(out)
    good = out[:need].copy()
    check_members(members_of(good.tobytes()), plain, MAX_BLOCK)
    for cap in (0, 1, need - 1):
        out[:] = 0x5A
        assert call(MAX_BLOCK, cap) == K.TS_ERR_INVALID_ARG
        assert nbytes.value == need and (out == 0x5A).all()
    out[:] = 0x5A
    assert call(MAX_BLOCK, need) == K.TS_OK
    assert np.array_equal(out[:need], good) and (out[need:] == 0x5A).all()
    for bad in (0, MAX_BLOCK + 1, 0xFFFFFFFF):
        assert call(bad, len(out)) == K.TS_ERR_INVALID_ARG
    before = stats(ctx)
    assert call(MAX_BLOCK, len(out), n=0) == K.TS_OK and (nbytes.value, count.value) == (0, 0)
    assert [a - b for a, b in zip(stats(ctx), before)] == [1, 0, 0, 0]
    assert L.ts_bgzf_deflate(None, src.ctypes.data, 10, 700, out.ctypes.data, len(out), C.byref(nbytes), C.byref(count)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bgzf_deflate(ctx, src.ctypes.data, 10, 700, out.ctypes.data, len(out), None, C.byref(count)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bgzf_deflate_stats(None, (C.c_uint64 * 4)()) == K.TS_ERR_INVALID_ARG
