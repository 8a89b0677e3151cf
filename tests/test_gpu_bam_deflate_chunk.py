"""ts_bam_chunk_gather_bgzf against ts_bam_chunk_gather on the gather scenarios of tests/test_gpu_bam_chunk.py: the members
that come back are valid BGZF (header, BSIZE, CRC32, ISIZE, at most 65 536 bytes each), inflate with zlib to exactly the
bytes the plain gather returns for the same table and pass bytes, and *plain_bytes and *n_passed agree with it.  Nothing
passing gives no member; a record larger than one payload runs over several members."""
import ctypes as C
import random
import zlib

import pytest
import torch

from tests import bamchunk as B
from tests import deflatecases
from tests.test_gpu_bam_chunk import assert_same_bytes, check_walk, env, gather_table, pass_patterns  # noqa: F401
from tests.test_gpu_bgzf_deflate import members_of

pytestmark = pytest.mark.gpu
PAYLOAD = 0xFF00


def gather_bgzf(env, table, d_pass, cap, payload=PAYLOAD, fill=0xA5):
    """-> (rc, host_out as the call left it, *bytes, *n_passed, *plain_bytes)"""
    out = C.create_string_buffer(bytes([fill]) * cap, cap) if cap else None
    nbytes, npassed, nplain = C.c_uint64(0xdead), C.c_uint64(0xdead), C.c_uint64(0xdead)
    rc = env.L.ts_bam_chunk_gather_bgzf(env.chunk.ptr, B.table_of(table), len(table), d_pass, payload, out, cap, C.byref(nbytes),
                                        C.byref(npassed), C.byref(nplain), None)
    return rc, (out.raw if cap else b""), nbytes.value, npassed.value, nplain.value


def inflate_members(data, payload):
    members = members_of(data)
    plain = b""
    for i, (deflated, crc, isize) in enumerate(members):
        piece = deflatecases.raw_inflate(deflated)
        assert len(piece) == isize and (isize == payload or i == len(members) - 1), i
        assert len(deflated) <= isize + 5, i
        assert crc == zlib.crc32(piece) & 0xFFFFFFFF, i
        plain += piece
    return plain, len(members)


def check_against_plain_gather(env, plain, table, pats, what, payload=PAYLOAD):
    K, chunk = env.K, env.chunk
    for name, p in pats.items():
        d_pass = torch.tensor(p, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ptr = C.c_void_p(d_pass.data_ptr())
        exp, kept = B.ref_gather(plain, table, p)
        rc, out, nbytes, npassed = chunk.gather(table, ptr, len(exp))
        assert (rc, out, nbytes, npassed) == (K.TS_OK, exp, len(exp), kept), (what, name)
        cap = len(exp) + 31 * (len(exp) // payload + 1)
        rc, got, zbytes, zpassed, zplain = gather_bgzf(env, table, ptr, cap, payload)
        assert (rc, zpassed, zplain) == (K.TS_OK, kept, len(exp)), (what, name, rc, zpassed, zplain, env.L.ts_last_error(env.ctx))
        if not exp:
            assert zbytes == 0 and got == b"\xa5" * cap, (what, name)       # nothing passes: no member
            continue
        assert got[zbytes:] == b"\xa5" * (cap - zbytes), (what, name)
        back, count = inflate_members(got[:zbytes], payload)
        assert count == -(-len(exp) // payload), (what, name)
        assert_same_bytes(back, exp, "%s, %s" % (what, name))


@pytest.mark.parametrize("n", [1, 64, 65, 3000])
def test_small_records(env, n):  # noqa: F811
    gen = random.Random(n)
    plain, table = gather_table(env, [gen.randrange(37, 300) for _ in range(n)], n)
    check_against_plain_gather(env, plain, table, pass_patterns(n, n), "n = %d" % n)


def test_many_members_per_gather(env):  # noqa: F811
    gen = random.Random(77)
    plain, table = gather_table(env, [gen.randrange(37, 300) for _ in range(3000)], 78)
    pats = {k: v for k, v in pass_patterns(3000, 79).items() if k in ("all", "random", "none")}
    check_against_plain_gather(env, plain, table, pats, "payload 700", payload=700)


def test_records_larger_than_one_payload(env):  # noqa: F811
    gen = random.Random(4)
    big = {3: 66000, 4: 131077, 40: 65536 + 37, 63: 300000}
    sizes = [gen.randrange(37, 300) for _ in range(192)]
    for p, s in big.items():
        sizes[64 + p] = s
    plain, table = gather_table(env, sizes, 5)
    pats = {"all": [1] * 192, "only the large": [int(i - 64 in big) for i in range(192)],
            "one large record alone": [int(i == 64 + 63) for i in range(192)], "all but the large": [int(i - 64 not in big) for i in range(192)]}
    check_against_plain_gather(env, plain, table, pats, "large records")


def test_capacity_arguments_and_counters(env):  # noqa: F811
    K, chunk = env.K, env.chunk
    gen = random.Random(21)
    plain, table = gather_table(env, [gen.randrange(37, 300) for _ in range(500)], 22)
    p = [gen.choice((0, 1)) for _ in table]
    exp, kept = B.ref_gather(plain, table, p)
    d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, len(p))
    assert d_pass
    B.to_device(d_pass, bytes(p))

    def stats():
        out = (C.c_uint64 * 4)()
        assert env.L.ts_bgzf_deflate_stats(env.ctx, out) == K.TS_OK
        return list(out)
    before = stats()
    rc, out, need, npassed, nplain = gather_bgzf(env, table, d_pass, len(exp) + 100)
    assert (rc, npassed, nplain) == (K.TS_OK, kept, len(exp)) and 0 < need <= len(exp) + 31 * -(-len(exp) // PAYLOAD)
    assert [a - b for a, b in zip(stats(), before)] == [1, -(-len(exp) // PAYLOAD), len(exp), need]
    good = out[:need]
    assert inflate_members(good, PAYLOAD)[0] == exp
    for cap in (0, need - 1):
        rc, out, nbytes, npassed, nplain = gather_bgzf(env, table, d_pass, cap)
        assert (rc, nbytes, npassed, nplain) == (K.TS_ERR_INVALID_ARG, need, kept, len(exp))
        assert out == b"\xa5" * cap                                                # host_out untouched
    rc, out, nbytes, _, _ = gather_bgzf(env, table, d_pass, need)
    assert (rc, nbytes, out) == (K.TS_OK, need, good)                              # the same bytes again
    for payload in (0, PAYLOAD + 1):
        assert gather_bgzf(env, table, d_pass, need, payload)[0] == K.TS_ERR_INVALID_ARG
    # nothing passes: no member, no deflate call
    B.to_device(d_pass, bytes(len(p)))
    before = stats()
    assert gather_bgzf(env, table, d_pass, 0) == (K.TS_OK, b"", 0, 0, 0)
    assert gather_bgzf(env, [], None, 0) == (K.TS_OK, b"", 0, 0, 0)
    assert stats() == before
    bad = list(table)
    bad[7] = (chunk.size() - 10,) + bad[7][1:]
    assert gather_bgzf(env, bad, d_pass, need)[0] == K.TS_ERR_INVALID_ARG
    n = C.c_uint64(0)
    assert env.L.ts_bam_chunk_gather_bgzf(None, None, 0, None, PAYLOAD, None, 0, C.byref(n), C.byref(n), C.byref(n), None) == K.TS_ERR_INVALID_ARG
