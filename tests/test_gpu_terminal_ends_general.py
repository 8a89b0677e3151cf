"""The per-side maxima of walkSegment (src/input.cpp:835-881) on the device for pattern sets the tiled kernel does not take:
ts_terminal_ends through the general kernels' ENDS walk (blockcall.hip: ts_terminal_ends_walk), ts_batch_terminal_ends on
general and on tiled tips batches, and ts_batch_download_blocks / ts_batch_segment_summary on general tips batches.  Expectations
are the CPU oracle's terminal blocks reduced per side (tests/endsets.py) and the blocks route of the same context
(ts_scan_segments_blocks: the blocks called on the device, downloaded, and reduced here) — an independent implementation."""
import ctypes as C

import numpy as np
import pytest

from tests import endsets as E
from tests import harness as H
from tests import readsets as R

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def env():
    import torch

    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input

    class Env:
        pass
    e = Env()
    e.torch, e.ta, e.K, e.L, e.user_input = torch, ta, K, K.lib(), user_input
    e.dev = torch.device("cuda", 0)
    return e


def teloscope(env, opts):
    return env.ta.Teloscope(env.user_input(opts, device=0))


def create(env, ctx, lens, abs_pos=None, tips=1):
    n = len(lens)
    arr = (C.c_uint64 * max(n, 1))(*lens)
    pos = (C.c_uint64 * max(n, 1))(*abs_pos) if abs_pos is not None else None
    b = env.L.ts_batch_create(ctx, arr, pos, n, tips, 0)
    assert b, env.L.ts_last_error(ctx)
    return b


def scan(env, ctx, b, segs):
    for i, s in enumerate(segs):
        assert env.L.ts_batch_upload(b, i, s) == env.K.TS_OK, env.L.ts_last_error(ctx)
    assert env.L.ts_batch_scan(b, None, None) == env.K.TS_OK, env.L.ts_last_error(ctx)


def batch_ends(env, ctx, b, segs):
    """Uploads, scans and reduces on the null stream, with the overflow protocol of ts_batch_read_pass; -> ((n, 2) uint32,
    whether the first status reported an overflow).  The 16 bytes behind the last pair must keep their fill value."""
    L, K, torch = env.L, env.K, env.torch
    n = len(segs)
    scan(env, ctx, b, segs)
    d_ends = torch.full((2 * n + 4,), FILL - (1 << 32), dtype=torch.int32, device=env.dev)
    torch.cuda.synchronize()
    p = C.c_void_p(d_ends.data_ptr())
    flag = C.c_int(7)
    assert L.ts_batch_terminal_ends(b, p, None) == K.TS_OK, L.ts_last_error(ctx)
    assert L.ts_batch_read_pass_status(b, C.byref(flag)) == K.TS_OK and flag.value in (0, 1)
    first = flag.value
    if first:
        assert L.ts_batch_sync(b) == K.TS_OK, L.ts_last_error(ctx)
        assert L.ts_batch_terminal_ends(b, p, None) == K.TS_OK, L.ts_last_error(ctx)
        assert L.ts_batch_read_pass_status(b, C.byref(flag)) == K.TS_OK and flag.value == 0
    torch.cuda.synchronize()
    got = d_ends.cpu().numpy().view(np.uint32)
    assert (got[2 * n:] == FILL).all()
    return got[:2 * n].reshape(n, 2).copy(), first


def blocks_route(tel, segs, abs_pos, with_counts=False):
    res = tel.scanSegmentsBlocksOnly(list(zip(segs, abs_pos)), tipsOnly=True, with_counts=with_counts)
    return res


def reduce_blocks(res, segs, abs_pos):
    return np.array([E.per_side(r.terminalBlocks, len(s), a) for r, s, a in zip(res, segs, abs_pos)], dtype=np.uint32).reshape(len(segs), 2)


def ends_stats(tel):
    return tel.terminal_ends_stats()


@pytest.mark.parametrize("flags", R.SETS, ids=R.SET_IDS)
def test_terminal_ends_of_a_general_set_are_reduced_on_the_device(env, flags):
    """Before the general ENDS walk there is no ts_terminal_ends_stats, and every group's blocks are downloaded and reduced on the
    host: out[1] stays 0 and out[2] grows."""
    tel = teloscope(env, E.options(flags))
    assert not tel.usesFastPath()
    segs, abs_pos = E.segments(flags)
    E.assert_classes(flags)
    before = ends_stats(tel)
    got = tel.terminalEnds(list(segs), list(abs_pos))
    after = ends_stats(tel)
    exp = E.oracle_ends(flags)
    assert got.shape == exp.shape and got.dtype == np.uint32
    bad = [(i, len(segs[i]), got[i].tolist(), exp[i].tolist()) for i in range(len(segs)) if got[i].tolist() != exp[i].tolist()]
    assert not bad, bad[:5]
    assert np.array_equal(got, reduce_blocks(blocks_route(tel, segs, abs_pos), segs, abs_pos))
    tiled, general, host, d2h = [a - z for a, z in zip(after, before)]
    # (these segments are one pipeline group: a group holds 256 MB of regions)
    assert (tiled, general, host) == (0, len(segs), 0)
    assert 8 * len(segs) <= d2h <= 8 * len(segs) + 64
    assert ends_stats(tel) == after                                 # the blocks route is not counted


@pytest.mark.parametrize("flags", R.SETS, ids=R.SET_IDS)
def test_batch_terminal_ends_on_a_general_tips_batch(env, flags):
    tel = teloscope(env, E.options(flags))
    ctx = tel._ctx.ptr
    segs, abs_pos = E.segments(flags)
    exp = E.oracle_ends(flags)
    E.assert_classes(flags)
    rb = (C.c_uint64 * 4)()
    assert env.L.ts_read_batch_stats(ctx, rb) == env.K.TS_OK
    rb0 = [int(x) for x in rb]
    before = ends_stats(tel)
    b = create(env, ctx, [len(s) for s in segs], abs_pos)
    try:
        got, first = batch_ends(env, ctx, b, segs)
        assert np.array_equal(got, exp)
        # the same lengths, the other content: the forward unit where the segment had no start side, random bases where it had
        rng = np.random.default_rng(29)
        unit = E.options(flags).canonical_fwd.encode()
        other = [R.random_bases(rng, len(s)) if e[0] else (unit * (len(s) // len(unit) + 1))[:len(s)] for s, e in zip(segs, exp)]
        got2, first2 = batch_ends(env, ctx, b, other)
        got3, first3 = batch_ends(env, ctx, b, segs)
    finally:
        env.L.ts_batch_destroy(b)
    assert np.array_equal(got2, reduce_blocks(blocks_route(tel, other, abs_pos), other, abs_pos))
    assert not np.array_equal(got2, got) and (got2 > 0).any()
    assert np.array_equal(got3, exp)
    after = ends_stats(tel)
    calls = 3 + first + first2 + first3                             # (a reduction is enqueued again after an overflow)
    assert after[1] - before[1] == calls * len(segs) and after[0] == before[0] and after[2] == before[2] and after[3] == before[3]
    # the D2H column of the batch's own counters: flag words only (four bytes per status call and per round of ts_batch_sync)
    assert env.L.ts_read_batch_stats(ctx, rb) == env.K.TS_OK
    scans, d2h = int(rb[0]) - rb0[0], int(rb[3]) - rb0[3]
    assert scans >= 3 and 4 * 3 <= d2h <= 64 * scans and d2h % 4 == 0
    for few in ([], [segs[60]], [segs[-N_TAIL]]):
        pos = [5] * len(few)
        b = create(env, ctx, [len(s) for s in few], pos)
        try:
            g, _ = batch_ends(env, ctx, b, few)
        finally:
            env.L.ts_batch_destroy(b)
        assert g.shape == (len(few), 2)
        if few:
            assert np.array_equal(g, reduce_blocks(blocks_route(tel, few, pos), few, pos))


N_TAIL = E.N_SHAPES                                                 # (segs[-N_TAIL]: the first shape, two blocks at the start side)


def test_batch_terminal_ends_on_a_tiled_tips_batch(env):
    opts = H.parse_cli("x" + E.TAIL)
    tel = teloscope(env, opts)
    assert tel.usesFastPath()
    ctx = tel._ctx.ptr
    segs = E.shapes(b"CCCTAA", b"TTAGGG")
    abs_pos = [1_000_003 * (i + 1) if i % 3 == 0 else 0 for i in range(len(segs))]
    exp = tel.terminalEnds(segs, abs_pos)
    assert (exp[:, 0] > 0).any() and (exp[:, 1] > 0).any() and exp[-1].tolist() == [0, 0]
    assert exp[5].tolist()[0] == 0 and exp[5].tolist()[1] > 0 and exp[6].tolist()[0] > 0 and exp[6].tolist()[1] == 0
    before = ends_stats(tel)
    b = create(env, ctx, [len(s) for s in segs], abs_pos)
    try:
        got, first = batch_ends(env, ctx, b, segs)
    finally:
        env.L.ts_batch_destroy(b)
    assert np.array_equal(got, exp)
    after = ends_stats(tel)
    assert after[0] - before[0] == len(segs) * (1 + first) and after[1] == before[1]
    # a full-scan batch has no terminal ends
    b = create(env, ctx, [len(s) for s in segs], abs_pos, tips=0)
    try:
        scratch = env.torch.zeros(2 * len(segs) + 4, dtype=env.torch.int32, device=env.dev)
        assert env.L.ts_batch_terminal_ends(b, C.c_void_p(scratch.data_ptr()), None) == env.K.TS_ERR_INVALID_ARG
        assert env.L.ts_batch_terminal_ends(None, C.c_void_p(scratch.data_ptr()), None) == env.K.TS_ERR_INVALID_ARG
        assert env.L.ts_batch_terminal_ends(b, None, None) == env.K.TS_ERR_INVALID_ARG
    finally:
        env.L.ts_batch_destroy(b)


def test_an_overflowed_scan_is_reported_and_the_second_reduction_is_right(env):
    opts = H.parse_cli("x " + R.OVERFLOW_SET + " -l 30")
    tel = teloscope(env, opts)
    ctx = tel._ctx.ptr
    segs = R.overflow_reads()
    abs_pos = [0] * len(segs)
    b = create(env, ctx, [len(s) for s in segs], abs_pos)
    try:
        got, first = batch_ends(env, ctx, b, segs)
    finally:
        env.L.ts_batch_destroy(b)
    assert first == 1
    exp = reduce_blocks(blocks_route(tel, segs, abs_pos), segs, abs_pos)
    assert np.array_equal(got, exp)
    assert any(e.tolist() != [0, 0] for e in exp) and any(e.tolist() == [0, 0] for e in exp)
    before = ends_stats(tel)
    assert np.array_equal(tel.terminalEnds(segs, abs_pos), exp)       # the host entry settles the overflow inside the group
    after = ends_stats(tel)
    assert after[1] - before[1] == len(segs) and after[2] == before[2]


def download_blocks(env, ctx, b, n):
    out = (env.K.SegmentOut * max(n, 1))()
    assert env.L.ts_batch_download_blocks(b, out) == env.K.TS_OK, env.L.ts_last_error(ctx)
    res = [env.ta.SegmentData(out[i], True) for i in range(n)]
    env.L.ts_free_segments(out, n)
    return res


BLOCK_FIELDS = ["start", "block_len", "block_label", "block_counts", "forward_count", "reverse_count", "canonical_count",
                "non_canonical_count", "total_covered", "fwd_covered", "can_covered", "has_valid_or"]


@pytest.mark.parametrize("flags", R.SETS, ids=R.SET_IDS)
def test_blocks_and_sums_of_a_general_tips_batch(env, flags):
    L, K, torch = env.L, env.K, env.torch
    tel = teloscope(env, E.options(flags))
    ctx = tel._ctx.ptr
    segs, abs_pos = E.segments(flags)
    n = len(segs)
    exp, exp_counts = blocks_route(tel, segs, abs_pos, with_counts=True)
    assert sum(len(r.terminalBlocks) for r in exp) >= 40 and any(len(r.terminalBlocks) == 2 for r in exp)
    assert any(c[1] for c in exp_counts) and all(c[0] == 0 for c in exp_counts)
    b = create(env, ctx, [len(s) for s in segs], abs_pos)
    try:
        scan(env, ctx, b, segs)
        got = download_blocks(env, ctx, b, n)
        d_sum = torch.full((4 * n + 2,), -3, dtype=torch.int64, device=env.dev)
        assert L.ts_batch_segment_summary(b, C.c_void_p(d_sum.data_ptr()), None) == K.TS_OK, L.ts_last_error(ctx)
        torch.cuda.synchronize()
        sums = d_sum.cpu().numpy()
        # ... and the ends after them, on the same scan
        d_ends = torch.zeros(2 * n, dtype=torch.int32, device=env.dev)
        assert L.ts_batch_terminal_ends(b, C.c_void_p(d_ends.data_ptr()), None) == K.TS_OK
        torch.cuda.synchronize()
        # the calls a general tips batch does not serve are still refused by name
        scratch = torch.zeros(4096, dtype=torch.uint8, device=env.dev)
        p = C.c_void_p(scratch.data_ptr())
        out = (K.SegmentOut * n)()
        for name, call in [("ts_batch_restrict", lambda: L.ts_batch_restrict(b, 0, 0)),
                           ("ts_batch_download", lambda: L.ts_batch_download(b, None, out)),
                           ("ts_batch_pack_shard", lambda: L.ts_batch_pack_shard(b, p, 4096, None)),
                           ("ts_batch_export", lambda: L.ts_batch_export(b, p, 16, p, None)),
                           ("ts_batch_set_emit", lambda: L.ts_batch_set_emit(b, 1))]:
            assert call() == K.TS_ERR_UNSUPPORTED, name
            assert name.encode() in L.ts_last_error(ctx), (name, L.ts_last_error(ctx))
        again = download_blocks(env, ctx, b, n)
    finally:
        L.ts_batch_destroy(b)
    for i, (g, a, e) in enumerate(zip(got, again, exp)):
        assert len(g.windows) == 0 and len(g.allMatches) == 0 and len(g.fwdMatches) == 0 and len(g.interstitialBlocks) == 0
        assert len(g.terminalBlocks) == len(e.terminalBlocks) == len(a.terminalBlocks), i
        for f in BLOCK_FIELDS:
            assert g.terminalBlocks[f].tolist() == e.terminalBlocks[f].tolist() == a.terminalBlocks[f].tolist(), (i, f)
    assert (sums[4 * n:] == -3).all()
    assert [tuple(int(x) for x in sums[4 * i:4 * i + 4]) for i in range(n)] == [tuple(c) for c in exp_counts]
    assert np.array_equal(d_ends.cpu().numpy().view(np.uint32).reshape(n, 2), E.oracle_ends(flags))


def test_two_tips_off_a_16_byte_boundary(env):
    """-t 400: segments up to 800 bases are one region, longer ones two tips, and the second tip of a 5 000-base segment starts
    off a 16-byte boundary — the strided form of the fused pass."""
    opts = H.parse_cli("x -p TTAGGG,TTAGG -t 400")
    tel = teloscope(env, opts)
    ctx = tel._ctx.ptr
    rng = np.random.default_rng(31)
    f, r = b"CCCTAA" * 60, b"TTAGGG" * 60
    rnd = lambda n: R.random_bases(rng, n)                         # noqa: E731
    segs = [b"TTAGGG" * 50, rnd(800), f + rnd(801 - 360), rnd(5000 - 360) + r,
            rnd(801 - 360) + f, r + rnd(5000 - 360),
            rnd(500) + r + rnd(5000 - 860), f + rnd(5000 - 360)]
    assert [len(s) for s in segs] == [300, 800, 801, 5000, 801, 5000, 5000, 5000]
    abs_pos = [0, 7, 0, 0, 11, 0, 0, 13]
    exp = reduce_blocks(blocks_route(tel, segs, abs_pos), segs, abs_pos)
    assert [e.tolist() != [0, 0] for e in exp] == [True, False, True, True, False, False, False, True]
    assert exp[3][1] > 0 and exp[3][0] == 0 and exp[7][0] > 0 and exp[7][1] == 0
    b = create(env, ctx, [len(s) for s in segs], abs_pos)
    try:
        got, _ = batch_ends(env, ctx, b, segs)
        blocks = download_blocks(env, ctx, b, len(segs))
    finally:
        env.L.ts_batch_destroy(b)
    assert np.array_equal(got, exp)
    assert np.array_equal(reduce_blocks(blocks, segs, abs_pos), exp)
    assert np.array_equal(tel.terminalEnds(segs, abs_pos), exp)
