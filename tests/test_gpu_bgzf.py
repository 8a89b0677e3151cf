"""ts_bgzf_inflate on the GPU against zlib: the clean grid of tests/test_inflate_core_cpu.py as some 3 000 members in one call,
and its damaged set one bad member per call among good ones.  The kernel compiles the decoder that test runs on the host
under sanitizers, so that file comes first in any job that runs this one.  These tests are here to see damaged input
rejected; none of them is meant to make the device fault."""
import random
import zlib

import numpy as np
import pytest

from tests.test_inflate_core_cpu import (BAD_CRC, BAD_DEFLATE, OK, SETTINGS, SIZES, contents, damaged_cases, deflate,
                                         zlib_verdict)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import teloscope_amd as ta
    from teloscope_amd.cli import parse_cli, user_input
    tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=0))
    yield tel._ctx.ptr
    del tel


def pack(members, gen, gap=True):
    """members: [(payload, isize, crc)] -> (compressed bytes, descriptors, output size, [dst_off]): payloads back to back at
    odd addresses, outputs in shuffled order with a few bytes between them."""
    comp, src = bytearray(b"\x5a"), []
    for payload, _, _ in members:
        src.append(len(comp))
        comp += payload
        if gap:
            comp += b"\xa5" * gen.randrange(0, 4)
    order = list(range(len(members)))
    gen.shuffle(order)
    dst, at = [0] * len(members), 0
    for i in order:
        at += gen.randrange(0, 20) if gap else 0
        dst[i] = at
        at += members[i][1]
    blocks = [(src[i], len(members[i][0]), members[i][1], members[i][2], dst[i]) for i in range(len(members))]
    return bytes(comp), blocks, at + 3, dst


def test_clean_grid_in_one_call(ctx):
    from teloscope_amd import _capi as K
    from teloscope_amd.bgzf import inflate_blocks
    members, plains, btypes = [], [], set()
    empty = (b"\x03\x00", 0, 0)
    for rep in range(8):
        data, far = contents(np.random.default_rng(100 + rep))
        for name, level, strategy in SETTINGS:
            for kind, plain in [(k, v[:n]) for k, v in data.items() for n in SIZES] + [("far_exact", far)]:
                payload = deflate(plain, level, strategy)
                if len(payload) > 65536:
                    continue
                btypes.add((payload[0] >> 1) & 3)
                members.append((payload, len(plain), zlib.crc32(plain) & 0xFFFFFFFF)); plains.append(plain)
                if len(members) % 7 == 0:
                    members.append(empty); plains.append(b"")
    assert btypes == {0, 1, 2} and len(members) >= 3000
    comp, blocks, cap, dst = pack(members, random.Random(5))
    out, (code, block) = inflate_blocks(ctx, comp, blocks, plain_cap=cap)
    assert (code, block) == (K.BGZF_OK, len(members))
    covered = np.zeros(cap, dtype=bool)
    for i, plain in enumerate(plains):
        assert out[dst[i]:dst[i] + len(plain)] == plain, (i, len(plain))
        covered[dst[i]:dst[i] + len(plain)] = True
    assert not np.frombuffer(out, dtype=np.uint8)[~covered].any(), "bytes between the members were written"


def test_damaged_members_get_zlibs_verdict(ctx):
    from teloscope_amd.bgzf import inflate_blocks
    cases, _ = damaged_cases()
    gen = random.Random(77)
    rng = np.random.default_rng(3)
    data, _ = contents(rng)
    good, good_plain = [], []
    for name, level, strategy in SETTINGS:
        for kind in ("dna", "qual", "bam", "one"):
            a = gen.randrange(0, 60000)
            plain = data[kind][a:a + gen.randrange(1, 3000)]
            good.append((deflate(plain, level, strategy), len(plain), zlib.crc32(plain) & 0xFFFFFFFF)); good_plain.append(plain)
    n_bad = {BAD_DEFLATE: 0, BAD_CRC: 0}
    for tag, payload, isize, crc in cases:
        want, _ = zlib_verdict(payload, isize, crc)
        picks = [gen.randrange(len(good)) for _ in range(99)]
        at = gen.randrange(100)
        members = [good[k] for k in picks]
        members.insert(at, (payload, isize, crc))
        comp, blocks, cap, dst = pack(members, gen)
        out, (code, block) = inflate_blocks(ctx, comp, blocks, plain_cap=cap)
        if want == OK:
            assert (code, block) == (OK, 100), tag
        else:
            assert (code, block) == (want, at), (tag, want, code, block, at)
            n_bad[want] += 1
        for i, k in enumerate(picks):
            j = i if i < at else i + 1
            assert out[dst[j]:dst[j] + len(good_plain[k])] == good_plain[k], (tag, j)
    assert n_bad[BAD_DEFLATE] >= 200 and n_bad[BAD_CRC] >= 200
