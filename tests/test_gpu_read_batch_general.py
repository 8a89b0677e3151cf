"""General tips batches through the C-ABI: ts_batch_create(..., tips_only = 1) on a context whose tips scans go to the general
kernels, then ts_batch_upload -> ts_batch_scan -> ts_batch_read_pass -> ts_batch_read_pass_status (-> ts_batch_sync and a second
pass after an overflow).  The pass bytes are compared with ts_filter_reads of the same context — the host route, an independent
implementation: it downloads the blocks and assembles SegmentData — and with the CPU oracle's read filter."""
import ctypes as C

import numpy as np
import pytest

from tests import harness as H
from tests import readsets as R

pytestmark = pytest.mark.gpu


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


def read_filter(env, flags):
    return env.ta.ReadTelomereFilter(env.user_input(R.options(flags), device=0))


def stats(env, ctx):
    out = (C.c_uint64 * 4)()
    assert env.L.ts_read_batch_stats(ctx, out) == env.K.TS_OK
    return [int(x) for x in out]


def create(env, ctx, lens):
    n = len(lens)
    arr = (C.c_uint64 * max(n, 1))(*lens)
    b = env.L.ts_batch_create(ctx, arr, None, n, 1, 0)
    assert b, env.L.ts_last_error(ctx)
    return b


def judge(env, ctx, b, reads):
    """Uploads the reads, scans and judges on the null stream; -> (pass bytes, whether the first pass overflowed)."""
    L, K, torch = env.L, env.K, env.torch
    n = len(reads)
    for i, r in enumerate(reads):
        assert L.ts_batch_upload(b, i, r) == K.TS_OK, L.ts_last_error(ctx)
    d_pass = torch.full((n + 16,), 7, dtype=torch.uint8, device=env.dev)
    torch.cuda.synchronize()
    flag = C.c_int(7)
    assert L.ts_batch_scan(b, None, None) == K.TS_OK, L.ts_last_error(ctx)
    assert L.ts_batch_read_pass(b, C.c_void_p(d_pass.data_ptr()), None) == K.TS_OK, L.ts_last_error(ctx)
    assert L.ts_batch_read_pass_status(b, C.byref(flag)) == K.TS_OK and flag.value in (0, 1)
    first = flag.value
    if first:
        assert L.ts_batch_sync(b) == K.TS_OK, L.ts_last_error(ctx)
        assert L.ts_batch_read_pass(b, C.c_void_p(d_pass.data_ptr()), None) == K.TS_OK
        assert L.ts_batch_read_pass_status(b, C.byref(flag)) == K.TS_OK and flag.value == 0
    torch.cuda.synchronize()
    got = d_pass.cpu().numpy()
    assert (got[n:] == 7).all()                                     # nothing behind the last read's byte is written
    assert set(got[:n].tolist()) <= {0, 1}
    return [bool(x) for x in got[:n]], first


@pytest.mark.parametrize("flags", R.SETS, ids=R.SET_IDS)
def test_pass_bytes_equal_the_host_route_and_the_oracle(env, flags):
    """Without general tips batches ts_batch_create returns NULL here ("unsupported parameter set")."""
    rf = read_filter(env, flags)
    ctx = rf._ctx.ptr
    assert env.L.ts_uses_fast_path(ctx) == 0 and env.L.ts_takes_text_input(ctx, 1) == 1
    reads = R.reads_for(flags)
    before = stats(env, ctx)
    b = create(env, ctx, [len(r) for r in reads])
    try:
        got, _ = judge(env, ctx, b, reads)
    finally:
        env.L.ts_batch_destroy(b)
    host = rf.matchesBatch(reads)
    exp = list(R.oracle_passes(flags))
    print("%s: %d of %d pass (first 60: %d, edge reads: %d)" % (flags, sum(exp), len(exp), sum(exp[:60]), sum(exp[60:])))
    assert got == host
    assert got == exp
    assert 0 < sum(exp[:60]) < 60 and 0 < sum(exp[60:]) < len(exp) - 60
    # nothing but flag words left the device: the segments were judged there, at most 64 bytes came back per scan
    after = stats(env, ctx)
    scans, judged, _, d2h = [a - z for a, z in zip(after, before)]
    assert scans >= 1 and judged == len(reads) * scans
    assert 0 < d2h <= 64 * scans


def test_dense_mixed_lengths_overflow_their_slots_and_rescan(env):
    rf = read_filter(env, R.OVERFLOW_SET)
    ctx = rf._ctx.ptr
    reads = R.overflow_reads()
    before = stats(env, ctx)
    b = create(env, ctx, [len(r) for r in reads])
    try:
        got, first = judge(env, ctx, b, reads)
    finally:
        env.L.ts_batch_destroy(b)
    after = stats(env, ctx)
    assert first == 1
    assert after[2] > before[2]                                     # ts_batch_sync rescanned
    assert after[0] - before[0] == 1 + (after[2] - before[2])
    host = rf.matchesBatch(reads)
    assert got == host
    assert 0 < sum(host) < len(host)


def test_a_batch_is_reused_with_other_input_and_small_batches_work(env):
    flags = R.SETS[0]
    rf = read_filter(env, flags)
    ctx = rf._ctx.ptr
    opts = R.options(flags)
    rng = np.random.default_rng(23)
    first = R.reads_for(flags)[:30]
    unit = opts.canonical_fwd.encode()
    # the same lengths, the other content: telomere where there was none and the reverse
    was = list(R.oracle_passes(flags))[:30]
    second = [R.random_bases(rng, len(r)) if p else (unit * (len(r) // len(unit) + 1))[:len(r)] for r, p in zip(first, was)]
    b = create(env, ctx, [len(r) for r in first])
    try:
        a1, _ = judge(env, ctx, b, first)
        a2, _ = judge(env, ctx, b, second)
        a3, _ = judge(env, ctx, b, first)
    finally:
        env.L.ts_batch_destroy(b)
    assert a1 == was == rf.matchesBatch(first)
    assert a2 == rf.matchesBatch(second) and a2 != a1
    assert a3 == a1
    for reads in ([], [first[0]], [first[1]]):
        b = create(env, ctx, [len(r) for r in reads])
        try:
            info = env.K.BatchInfo()
            assert env.L.ts_batch_get_info(b, C.byref(info)) == env.K.TS_OK
            assert info.n_segments == len(reads) and info.total_bases == sum(len(r) for r in reads) and info.n_windows == 0
            assert info.input_bytes >= sum((len(r) + 15) // 16 * 16 for r in reads)
            got, _ = judge(env, ctx, b, reads)
        finally:
            env.L.ts_batch_destroy(b)
        assert got == (rf.matchesBatch(reads) if reads else [])


def test_regions_of_a_full_scan_context_follow_the_terminal_limit(env):
    """A ts_create context with -t 400: segments up to 800 bases are one region, longer ones two tips (the second starts off a
    16-byte boundary).  Pass bytes against n_terminal_blocks != 0 of ts_scan_segments_blocks on the same tips-only segments."""
    opts = H.parse_cli("x -p TTAGGG,TTAGG -t 400")
    tel = env.ta.Teloscope(env.user_input(opts, device=0))
    ctx = tel._ctx.ptr
    rng = np.random.default_rng(31)
    f, r = b"CCCTAA" * 60, b"TTAGGG" * 60                          # 360 bases: the forward unit counts at the start, the reverse one at the end
    rnd = lambda n: R.random_bases(rng, n)                         # noqa: E731
    segs = [b"TTAGGG" * 50, rnd(800), f + rnd(801 - 360), rnd(5000 - 360) + r,         # one region, one region, telomere at one end only
            rnd(801 - 360) + f, r + rnd(5000 - 360),                                    # ... in the orientation that does not count there
            rnd(500) + r + rnd(5000 - 860), f + rnd(5000 - 360)]                        # between the tips: not scanned; the start tip
    assert [len(s) for s in segs] == [300, 800, 801, 5000, 801, 5000, 5000, 5000]
    b = create(env, ctx, [len(s) for s in segs])
    try:
        got, _ = judge(env, ctx, b, segs)
    finally:
        env.L.ts_batch_destroy(b)
    exp = [len(sd.terminalBlocks) != 0 for sd in tel.scanSegmentsBlocksOnly([(s, 0) for s in segs], tipsOnly=True)]
    assert got == exp
    assert got == [True, False, True, True, False, False, False, True]


def test_other_batch_calls_are_refused_by_name(env):
    L, K = env.L, env.K
    flags = R.SETS[3]
    rf = read_filter(env, flags)
    ctx = rf._ctx.ptr
    reads = R.reads_for(flags)[:12]
    b = create(env, ctx, [len(r) for r in reads])
    try:
        scratch = env.torch.zeros(4096, dtype=env.torch.uint8, device=env.dev)
        p = C.c_void_p(scratch.data_ptr())
        out = (K.SegmentOut * len(reads))()
        calls = [("ts_batch_restrict", lambda: L.ts_batch_restrict(b, 0, 0)),
                 ("ts_batch_download", lambda: L.ts_batch_download(b, None, out)),
                 ("ts_batch_pack_shard", lambda: L.ts_batch_pack_shard(b, p, 4096, None)),
                 ("ts_batch_export", lambda: L.ts_batch_export(b, p, 16, p, None)),
                 ("ts_batch_set_emit", lambda: L.ts_batch_set_emit(b, 1))]
        for name, call in calls:
            assert call() == K.TS_ERR_UNSUPPORTED, name
            assert name.encode() in L.ts_last_error(ctx), (name, L.ts_last_error(ctx))
        assert L.ts_batch_matches_ptr(b) is None
        assert b"ts_batch_matches_ptr" in L.ts_last_error(ctx)
        got, _ = judge(env, ctx, b, reads)
        for name, call in calls:                                    # ... and after a scan
            assert call() == K.TS_ERR_UNSUPPORTED, name
        assert L.ts_batch_matches_ptr(b) is None
        again, _ = judge(env, ctx, b, reads)
    finally:
        L.ts_batch_destroy(b)
    assert got == again == list(R.oracle_passes(flags))[:12]


def test_only_flag_words_leave_the_device(env):
    """ts_read_batch_stats around three judged batches: every read is judged on the device, and what comes back is the flag word
    of each status call — no record, no block, no per-read sum."""
    flags = R.SETS[4]
    rf = read_filter(env, flags)
    ctx = rf._ctx.ptr
    reads = R.reads_for(flags)
    assert stats(env, ctx) == [0, 0, 0, 0]
    b = create(env, ctx, [len(r) for r in reads])
    try:
        for _ in range(3):
            got, first = judge(env, ctx, b, reads)
            assert first == 0 and got == list(R.oracle_passes(flags))
    finally:
        env.L.ts_batch_destroy(b)
    scans, judged, rescans, d2h = stats(env, ctx)
    assert (scans, judged, rescans) == (3, 3 * len(reads), 0)
    assert d2h == 4 * scans <= 64 * scans
    assert rf.matchesBatch(reads) == got and stats(env, ctx) == [scans, judged, rescans, d2h]      # the host route is not counted
