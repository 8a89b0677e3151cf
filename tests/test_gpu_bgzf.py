"""ts_bgzf_inflate on the GPU against zlib: the clean grid of tests/test_inflate_core_cpu.py as some 3 000 members in one call,
and its damaged set one bad member per call among good ones; then the handmade streams of tests/deflategen.py, which no
encoder on this machine emits and which zlib's decoder has classed: each accepted list in one call (one match at every place
of a batch and every distance around the 64 bytes the wave writes at a time, chains of matches that copy each other, batches
of 64 longest matches, members of up to eight blocks, code-length sets behind the lookups), each member that breaks one
table rule alone among accepted ones, stored members of 0..130 bytes at every output alignment for the CRC's clipped
slices, and the chains once more through the resident chunk.  Streams of third-party encoders (libdeflate, igzip, zopfli)
are not among them.  The kernel compiles the decoder that tests/test_inflate_core_cpu.py runs on the host under sanitizers,
on these same streams, so that file comes first in any job that runs this one.  These tests are here to see valid input
decoded and damaged input rejected; none of them is meant to make the device fault."""
import random
import zlib

import numpy as np
import pytest

from tests import deflategen
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


# ------------------------------------------------------------------------------------- handmade streams (tests/deflategen.py)
@pytest.mark.parametrize("name", deflategen.ACCEPTED)
def test_handmade_list_in_one_call(ctx, name):
    """Every member's bytes are the ones its tokens stand for (which zlib's decoder gave too, when the list was built)."""
    from teloscope_amd import _capi as K
    from teloscope_amd.bgzf import inflate_blocks
    cases, plains = deflategen.cases(name), deflategen.plains(name)
    comp, blocks, cap, dst = pack([(p, n, c) for _, p, n, c in cases], random.Random(11))
    out, (code, block) = inflate_blocks(ctx, comp, blocks, plain_cap=cap)
    assert (code, block) == (K.BGZF_OK, len(cases)), (code, block, cases[min(block, len(cases) - 1)][0])
    covered = np.zeros(cap, dtype=bool)
    wrong = []
    for i, (tag, _, isize, _) in enumerate(cases):
        assert len(plains[tag]) == isize
        if out[dst[i]:dst[i] + isize] != plains[tag]:
            wrong.append(tag)
        covered[dst[i]:dst[i] + isize] = True
    assert not wrong, (len(wrong), wrong[:20])
    assert not np.frombuffer(out, dtype=np.uint8)[~covered].any(), "bytes between the members were written"


def test_broken_table_rules_get_zlibs_verdict(ctx):
    """Each member of tables_bad alone among 20 accepted handmade members: (zlib's class, its index), the others intact."""
    from teloscope_amd.bgzf import inflate_blocks
    gen = random.Random(78)
    good = []
    for name in deflategen.ACCEPTED:
        plains = deflategen.plains(name)
        small = [(p, n, c, plains[tag]) for tag, p, n, c in deflategen.cases(name) if n <= 3000]
        good += gen.sample(small, min(40, len(small)))
    assert len(good) >= 150
    n_bad = 0
    for tag, payload, isize, crc in deflategen.cases("tables_bad"):
        want, _ = zlib_verdict(payload, isize, crc)
        picks = [gen.randrange(len(good)) for _ in range(20)]
        at = gen.randrange(21)
        members = [good[k][:3] for k in picks]
        members.insert(at, (payload, isize, crc))
        comp, blocks, cap, dst = pack(members, gen)
        out, (code, block) = inflate_blocks(ctx, comp, blocks, plain_cap=cap)
        if want == OK:
            assert (code, block) == (OK, 21), tag
            assert out[dst[at]:dst[at] + isize] == deflategen.plains("tables_bad")[tag], tag
        else:
            assert want == BAD_DEFLATE and (code, block) == (want, at), (tag, want, code, block, at)
            n_bad += 1
        for i, k in enumerate(picks):
            j = i if i < at else i + 1
            assert out[dst[j]:dst[j] + good[k][1]] == good[k][3], (tag, j)
    assert n_bad >= 200


def crc_grid_call():
    """Stored members of 0..130 bytes, each at the 16 alignments of its first output byte (the buffer itself is aligned):
    (compressed, descriptor array, capacity, [plain])."""
    from teloscope_amd.bgzf import BLOCK_DT
    gen = random.Random(79)
    cases, plains = deflategen.cases("crc_grid"), deflategen.plains("crc_grid")
    members = [(tag, p, n, c, a) for tag, p, n, c in cases for a in range(16)]
    gen.shuffle(members)
    comp, at = bytearray(b"\x5a"), 0
    arr = np.zeros(len(members), dtype=BLOCK_DT)
    for i, (tag, p, n, c, a) in enumerate(members):
        at = (at + 15) // 16 * 16 + 16 * gen.randrange(2) + a
        arr[i] = (len(comp), len(p), n, c, 0, at)
        comp += p + b"\xa5" * gen.randrange(0, 4)
        at += n
    return bytes(comp), arr, at + 3, [plains[m[0]] for m in members]


def test_crc_at_every_size_and_alignment(ctx):
    from teloscope_amd import _capi as K
    from teloscope_amd.bgzf import inflate_blocks
    comp, arr, cap, plains = crc_grid_call()
    assert len(arr) == 131 * 16 and {(int(n), int(d) % 16) for n, d in zip(arr["isize"], arr["dst_off"])} == \
        {(n, a) for n in range(131) for a in range(16)}
    out, (code, block) = inflate_blocks(ctx, comp, arr, plain_cap=cap)
    assert (code, block) == (K.BGZF_OK, len(arr))
    covered = np.zeros(cap, dtype=bool)
    for i, plain in enumerate(plains):
        d = int(arr["dst_off"][i])
        assert out[d:d + len(plain)] == plain, (len(plain), d % 16)
        covered[d:d + len(plain)] = True
    assert not np.frombuffer(out, dtype=np.uint8)[~covered].any(), "bytes between the members were written"
    # one wrong CRC per call, every member in turn
    for i in range(len(arr)):
        bad = arr.copy()
        bad["crc"][i] ^= np.uint32(1 << (i % 32))
        _, (code, block) = inflate_blocks(ctx, comp, bad, plain_cap=cap)
        assert (code, block) == (K.BGZF_BAD_CRC, i), (code, block, i, int(arr["isize"][i]), int(arr["dst_off"][i]) % 16)


def test_chains_through_a_resident_chunk(ctx):
    """The chains list as one fill of a ts_bam_chunk: Chunk.fill asserts the status and that the chunk reads back as the
    concatenation of the members' bytes."""
    from tests import bamchunk as B
    cases, plains = deflategen.cases("chains"), deflategen.plains("chains")
    comp, descs, plain = bytearray(), [], bytearray()
    for tag, p, n, c in cases:
        descs.append((len(comp), len(p), n, c, len(plain)))
        comp += p
        plain += plains[tag]
    chunk = B.Chunk(ctx, len(comp) + 64, len(plain) + 64)
    try:
        assert chunk.fill(bytes(plain), (bytes(comp), descs)) == bytes(plain)
    finally:
        chunk.close()
