"""Reused device state with CHANGING input: every object the library keeps on the device from one scan to the next — the
context's BufferPool blocks (not zero-filled) and pinned landing slots, a batch's regions, window records, tile directory,
chain summaries and visible-record regions, a shard slot's bound message, a read batch's read table and overflow flag — is
given a different input on every step here, and every step is compared with the oracle for THAT step's input.

On a repeat of the same bytes, a scan that forgets to clear some state, or a buffer overwritten while a reader still needs
it, gives the right answer by accident; the other suites rescan what they scanned before.  So the sequences below start
with a poison (dense telomeric repeats in every pooled buffer), go on with smaller, tiny and larger calls, and come back to
an earlier input at the end."""
import ctypes as C

import numpy as np
import pytest

from tests import harness as H
from tests import seqgen
from tests.backends import (BLOCK_FIELDS, WINDOW_FIELDS, OracleBackend, OracleReadFilter, ProductReadFilter,
                            assert_segment_equal, assert_visible_view_equal, segment_as_dict)
from tests.test_gpu_parity import PUSH_ORDER_GRID, WIDE_GRID
from tests.test_gpu_shard_results import _fill
from tests.test_gpu_terminal_ends import per_side

pytestmark = pytest.mark.gpu

HEADLINE = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -m -i"
GENERAL = "-p TTAGGG,TTAGG -w 1000 -s 500 -r -g -e -m -i"
TIPS = "-t 300"
HOST_SETS = [HEADLINE, GENERAL, PUSH_ORDER_GRID[0], WIDE_GRID[0], TIPS]

# segment lengths of the steps of a host sequence: the poison is above the packed-upload threshold (1 MB), the smaller call
# 55-95 % of it (BufferPool::take hands back a block within 2x of the request: the poison's blocks), the tiny call below the
# threshold (plain upload), the larger call beyond the poison (fresh blocks).  Lengths avoid multiples of 16 and of the tiles.
POISON_LENS = [1_200_007, 650_001, 333_331, 120_013, 9_999]
SMALLER_LENS = [801_001, 0, 555_557, 230_017, 47_999, 123, 1_001]
TINY_LENS = [50_001, 3_333, 17, 0]
LARGER_LENS = [2_000_003, 1_100_011, 333_337]


def _revcom(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _units(opts):
    pats = [opts.canonical_fwd, opts.canonical_rev] + list(opts.raw_patterns or [])
    return sorted(set(pats + [_revcom(p) for p in pats]))


def _poison(rng, opts, lens):
    """Almost nothing but repeats of the canonical and of the other patterns (both strands), runs of 50-400 units with 1 %
    point mutations."""
    units = _units(opts)
    out = []
    for n in lens:
        parts, have = [], 0
        while have < n:
            u = units[int(rng.integers(0, len(units)))]
            run = seqgen.repeat_array(u, int(rng.integers(50, 400)))
            parts.append(run)
            have += len(run)
        s = seqgen.mutate(rng, np.concatenate(parts)[:n] if parts else np.zeros(0, np.uint8), 0.01)
        out.append(s.tobytes())
    return out


def _sparse(rng, opts, lens):
    """Random sequence with a telomere at a few ends, an interstitial array in the longest segment, a few IUPAC codes and a
    run of N that reaches a segment's end."""
    out = []
    longest = int(np.argmax(lens)) if len(lens) else -1
    for i, n in enumerate(lens):
        s = bytearray(seqgen.random_dna(rng, n).tobytes())
        if n >= 4000 and i % 3 == 0:
            u = seqgen.mutate(rng, seqgen.repeat_array(opts.canonical_fwd, int(rng.integers(40, 300))), 0.02).tobytes()[:n // 2]
            s[:len(u)] = u
        if n >= 4000 and i % 4 == 1:
            u = seqgen.mutate(rng, seqgen.repeat_array(opts.canonical_rev, int(rng.integers(40, 300))), 0.02).tobytes()[:n // 2]
            s[n - len(u):] = u
        if i == longest and n > 100_000:
            a = int(rng.integers(20_000, n - 20_000))
            s[a:a + 1200] = seqgen.repeat_array(opts.canonical_rev, 200).tobytes()
            for at in rng.integers(0, n, size=3):
                s[int(at)] = ord("R")
        if n >= 1000 and i % 5 == 2:
            s[n - 150:] = b"N" * 150                          # an N run touching the segment's end
        out.append(bytes(s))
    return out


def _assert_windows_blocks(sd, exp, ctx):
    gw, ew = sd.windows, exp["windows"]
    assert len(gw) == len(ew), "%s windows: %d vs %d" % (ctx, len(gw), len(ew))
    for f in WINDOW_FIELDS:
        assert np.array_equal(gw[f], ew[f]), "%s windows.%s differs" % (ctx, f)
    for name, g in (("terminal_blocks", sd.terminalBlocks), ("interstitial_blocks", sd.interstitialBlocks)):
        e = exp[name]
        assert len(g) == len(e), "%s %s: %d vs %d" % (ctx, name, len(g), len(e))
        for f in BLOCK_FIELDS:
            assert np.array_equal(g[f], e[f]), "%s %s.%s differs" % (ctx, name, f)


def _expected_counts(exp, tips):
    if tips:
        return (0, len(exp["fwd_matches"]) + len(exp["rev_matches"]), len(exp["fwd_matches"]))
    return (len(exp["windows"]), len(exp["all_matches"]), len(exp["canonical_matches"]), len(exp["fwd_matches"]))


def _host_context(cli):
    import teloscope_amd as ta
    from teloscope_amd.cli import parse_cli, user_input
    opts = parse_cli("x.fa " + cli)
    return opts, ta.Teloscope(user_input(opts, device=0))


# ------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("cli", HOST_SETS)
def test_host_entry_points_on_one_context_follow_changing_input(cli):
    """One Teloscope, five calls: poison, smaller (the poison's pooled blocks come back), tiny (plain upload), larger (fresh
    blocks), the smaller call's input again — each through a different entry point, each equal to the oracle."""
    opts, tel = _host_context(cli)
    tips = bool(opts.ultra_fast)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(sum(map(ord, cli)))
    poison = _poison(rng, opts, POISON_LENS)
    smaller = _sparse(rng, opts, SMALLER_LENS)
    tiny = _sparse(rng, opts, TINY_LENS)
    larger = _sparse(rng, opts, LARGER_LENS)
    assert sum(POISON_LENS) >= 2 << 20 and 0.55 < sum(SMALLER_LENS) / sum(POISON_LENS) < 0.95
    assert sum(TINY_LENS) < 1 << 20 and sum(LARGER_LENS) > sum(POISON_LENS)

    def full_call(seqs, flags, step):
        segs = [(s, 1000 * i + 7, f) for i, (s, f) in enumerate(zip(seqs, flags))]
        got = tel.scanSegments(segs)
        for i, (s, a, f) in enumerate(segs):
            assert_segment_equal(segment_as_dict(got[i]), orac.scan_segment(s, a, f), f, ctx="%s: %s segment %d" % (cli, step, i))

    def blocks_call(seqs, step):
        got, cnt = tel.scanSegmentsBlocksOnly([(s, 31 * i) for i, s in enumerate(seqs)], tipsOnly=tips, with_counts=True)
        for i, s in enumerate(seqs):
            exp = orac.scan_segment(s, 31 * i, tips)
            ctx = "%s: %s segment %d (blocks only)" % (cli, step, i)
            _assert_windows_blocks(got[i], exp, ctx)
            want = _expected_counts(exp, tips)
            assert tuple(cnt[i][:len(want)] if not tips else (cnt[i][0], cnt[i][1], cnt[i][3])) == want, ctx

    def ends_call(seqs, step):
        abs_pos = [0 if i % 2 else 5_000_011 * i for i in range(len(seqs))]
        got = tel.terminalEnds(seqs, abs_pos)
        for i, s in enumerate(seqs):
            exp = per_side(orac.scan_segment(s, abs_pos[i], True)["terminal_blocks"], len(s), abs_pos[i])
            assert list(got[i]) == exp, "%s: %s segment %d terminal ends %s vs %s" % (cli, step, i, list(got[i]), exp)

    full_call(poison, [tips] * len(poison), "poison")
    if tips:
        ends_call(smaller, "smaller")
    full_call(smaller, [tips] * len(smaller), "smaller")
    full_call(tiny, [i % 2 == 1 for i in range(len(tiny))], "tiny, full and tips-only mixed")
    blocks_call(larger, "larger")
    blocks_call(smaller, "smaller again")
    if tips:
        ends_call(poison, "poison again")
        ends_call(smaller, "smaller again")
    else:
        full_call(smaller, [False] * len(smaller), "smaller again")
    tel.close()


@pytest.mark.parametrize("cli", ["--fastq-subset -l 42", "--fastq-subset -p TTAGGG,TTAGG"])
def test_read_filter_on_one_context_follows_changing_reads(cli):
    """ReadTelomereFilter, one context: all-telomeric reads (> 2 MB), then random reads with telomeres at some ends, a tiny
    batch, a larger one and the second batch again — pass bits equal to the oracle's at every step."""
    opts = H.parse_cli(cli)
    rf, orac = ProductReadFilter(opts), OracleReadFilter(opts)
    rng = np.random.default_rng(17)
    fwd, rev = opts.canonical_fwd, opts.canonical_rev

    def telomeric(n):
        return [seqgen.mutate(rng, seqgen.repeat_array(fwd if i % 2 else rev, int(rng.integers(700, 1000))), 0.01).tobytes()
                for i in range(n)]

    def sparse(n, lo, hi):
        reads = []
        for i in range(n):
            body = seqgen.random_dna(rng, int(rng.integers(lo, hi))).tobytes()
            if i % 3 == 0:
                body = (fwd * int(rng.integers(3, 40))).encode() + body
            elif i % 3 == 1:
                body = body + (rev * int(rng.integers(3, 40))).encode()
            reads.append(body)
        return reads

    poison = telomeric(500)
    second = sparse(400, 1000, 7000)
    steps = [("poison", poison), ("second", second), ("tiny", sparse(25, 100, 900)), ("larger", sparse(700, 2000, 8000)),
             ("second again", second)]
    assert sum(map(len, poison)) > 2 << 20 and sum(map(len, second)) < sum(map(len, poison))
    for name, reads in steps:
        got, exp = rf.filter(reads), orac.filter(reads)
        assert got == exp, "%s: %s: %d reads differ" % (cli, name, sum(a != b for a, b in zip(got, exp)))
        if name != "poison":
            assert 0 < sum(exp) < len(exp), name
    assert all(orac.filter(poison))


# ------------------------------------------------------------------------------------------------------------------- B
def _download(L, b, n, full):
    from teloscope_amd import _capi as K
    out = (K.SegmentOut * n)()
    rc = L.ts_batch_download(b, None, out) if full else L.ts_batch_download_blocks(b, out)
    return rc, out


def test_device_batch_rescanned_with_new_bytes():
    """One ts_batch, five steps of new contents through ts_batch_upload: scan, sync, download or download_blocks, emit flipped
    between steps; the second step overflows the match capacity (sync regrows and rescans), the third is sparse."""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    L = K.lib()
    opts, tel = _host_context(HEADLINE)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(5)
    lens = [600_001, 0, 333_333, 77_777, 4_099]
    n = len(lens)
    cap = 20_000
    b = L.ts_batch_create(tel._ctx.ptr, (C.c_uint64 * n)(*lens), None, n, 0, cap)
    assert b, tel._ctx.error()
    steps = [("sparse", _sparse(rng, opts, lens), 1, True), ("poison", _poison(rng, opts, lens), 0, False),
             ("sparse after overflow", _sparse(rng, opts, lens), 1, True), ("sparse 2", _sparse(rng, opts, lens), 0, False),
             ("sparse 3", _sparse(rng, opts, lens), 1, False)]
    info = K.BatchInfo()
    try:
        for name, seqs, emit, full in steps:
            assert L.ts_batch_set_emit(b, emit) == 0
            for i, s in enumerate(seqs):
                assert L.ts_batch_upload(b, i, s) == 0, tel._ctx.error()
            assert L.ts_batch_scan(b, None, None) == 0, tel._ctx.error()
            assert L.ts_batch_sync(b) == 0, tel._ctx.error()
            L.ts_batch_get_info(b, C.byref(info))
            if name == "poison":
                assert info.n_matches > cap and info.match_capacity >= info.n_matches, (info.n_matches, info.match_capacity)
            rc, out = _download(L, b, n, full)
            assert rc == 0, tel._ctx.error()
            for i, s in enumerate(seqs):
                exp = orac.scan_segment(s, 0, False)
                ctx = "%s segment %d (emit %d, %s)" % (name, i, emit, "download" if full else "download_blocks")
                if full:
                    assert_segment_equal(segment_as_dict(ta.SegmentData(out[i], False)), exp, False, ctx=ctx)
                else:
                    _assert_windows_blocks(ta.SegmentData(out[i], False), exp, ctx)
            L.ts_free_segments(out, n)
    finally:
        L.ts_batch_destroy(b)


def test_hip_shard_results_adopted_step_after_step():
    """distributed.HipShard (bind_results + export) on two parts of a plan with a small match capacity, five steps of new
    input (one overflowing), emit flipped between steps: each step's arrays adopted and downloaded equal the oracle, and
    ts_batch_matches_ptr of the adopted batch is the dense stream it adopted."""
    import torch
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd import distributed as D
    L = K.lib()
    dev = torch.device("cuda", 0)
    opts, tel = _host_context(HEADLINE)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(6)
    lens = [700_001, 12_345, 0, 250_003]
    n = len(lens)
    plan = D.ShardPlan(tel, lens, world=2, match_capacity=20_000)
    shards = [D.HipShard(plan, p, dev, slots=1) for p in range(2)]
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    steps = [("sparse", _sparse(rng, opts, lens)), ("poison", _poison(rng, opts, lens)), ("sparse after overflow", _sparse(rng, opts, lens)),
             ("sparse 2", _sparse(rng, opts, lens)), ("poison 2", _poison(rng, opts, lens))]
    try:
        for k, (name, seqs) in enumerate(steps):
            buf = _fill(plan, seqs, dev)
            ws, ss, ds, counts = [], [], [], []
            for p, hs in enumerate(shards):
                assert L.ts_batch_set_emit(hs.batches[0], k % 2) == 0
                r = plan.ranges[p]
                local = buf[r.input_begin:r.input_end].clone()
                hs.scan(local.data_ptr(), sptr, 0)
                m = hs.finish(local.data_ptr(), sptr, 0)
                ws.append(hs.windows[0]); ss.append(hs.stats[0]); ds.append(hs.dense[0][:m])
                counts.append(m)
            a = D.Assembled(torch.cat(ws), torch.cat(ss), torch.cat(ds), sum(counts), counts)
            if name == "poison":
                assert sum(counts) > 20_000
            b = D.adopt(plan, a)
            try:
                assert L.ts_batch_matches_ptr(b) == a.dense.data_ptr(), "%s: the adopted dense stream has no raw view" % name
                rc, out = _download(L, b, n, k % 2 == 0)
                assert rc == 0, tel._ctx.error()
                for i, s in enumerate(seqs):
                    exp = orac.scan_segment(s, 0, False)
                    ctx = "HipShard %s segment %d" % (name, i)
                    if k % 2 == 0:
                        assert_segment_equal(segment_as_dict(ta.SegmentData(out[i], False)), exp, False, ctx=ctx)
                    else:
                        _assert_windows_blocks(ta.SegmentData(out[i], False), exp, ctx)
                L.ts_free_segments(out, n)
            finally:
                L.ts_batch_destroy(b)
    finally:
        for hs in shards:
            hs.close()
        plan.close()


# ------------------------------------------------------------------------------------------------------------------- C
def test_read_batch_rescanned_with_new_reads():
    """ts_batch_read_pass on one read batch (benchlib/reads.py's route), the same read lengths with new contents every step:
    a sparse step, an all-telomeric step that overflows the 4 096-record capacity (reported, nothing judged; sync, pass
    again), then clean steps whose status reads 0 on the first pass — every step's pass bytes equal to the oracle's."""
    import torch
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("--fastq-subset -l 42")
    rf = ta.ReadTelomereFilter(user_input(opts, device=0))
    orac = OracleReadFilter(opts)
    L = K.lib()
    rng = np.random.default_rng(23)
    lens = [int(x) for x in rng.integers(1500, 6000, size=300)]
    n = len(lens)
    b = L.ts_batch_create(rf._ctx.ptr, (C.c_uint64 * n)(*lens), None, n, 1, 4096)
    assert b
    info = K.BatchInfo()
    L.ts_batch_get_info(b, C.byref(info))
    dev = torch.device("cuda", 0)
    offs = [int(L.ts_batch_segment_offset(b, i)) for i in range(n)]
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def sparse():
        reads = []
        for i, ln in enumerate(lens):
            s = bytearray(seqgen.random_dna(rng, ln).tobytes())
            if i % 4 == 0:
                s[:300] = b"CCCTAA" * 50
            elif i % 4 == 1:
                s[ln - 300:] = b"TTAGGG" * 50
            reads.append(bytes(s))
        return reads

    def dense():
        return [seqgen.mutate(rng, seqgen.repeat_array("TTAGGG" if i % 2 else "CCCTAA", ln // 6 + 1), 0.01).tobytes()[:ln]
                for i, ln in enumerate(lens)]

    steps = [("sparse", sparse(), None), ("dense", dense(), True), ("clean after overflow", sparse(), False),
             ("clean 2", sparse(), False)]
    flag = C.c_int(0)
    try:
        for name, reads, must_overflow in steps:
            buf = torch.zeros(int(info.input_bytes), dtype=torch.uint8, device=dev)
            for off, r in zip(offs, reads):
                buf[off:off + len(r)] = torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev)
            d_pass = torch.full((n + 16,), 7, dtype=torch.uint8, device=dev)
            assert L.ts_batch_scan(b, C.c_void_p(buf.data_ptr()), sptr) == 0
            assert L.ts_batch_read_pass(b, C.c_void_p(d_pass.data_ptr()), sptr) == 0
            assert L.ts_batch_read_pass_status(b, C.byref(flag)) == 0
            if must_overflow is not None:
                assert flag.value == int(must_overflow), (name, flag.value)
            if flag.value:
                assert (d_pass[:n] == 7).all(), name                              # nothing was judged
                assert L.ts_batch_sync(b) == 0
                assert L.ts_batch_read_pass(b, C.c_void_p(d_pass.data_ptr()), sptr) == 0
                assert L.ts_batch_read_pass_status(b, C.byref(flag)) == 0 and flag.value == 0, name
            exp = orac.filter(reads)
            assert [bool(x) for x in d_pass[:n].cpu().numpy()] == exp, name
            assert sum(exp) > 0
    finally:
        L.ts_batch_destroy(b)


# ------------------------------------------------------------------------------------------------------------------- D
def _shard_setup(cli, lens, slots, world=2):
    import torch
    from teloscope_amd import distributed as D
    dev = torch.device("cuda", 0)
    opts, tel = _host_context(cli)
    plan = D.ShardPlan(tel, lens, world=world)
    shards = [D.PackedShard(plan, p, dev, slots=slots) for p in range(world)]
    return dev, opts, tel, plan, shards


def _locals(plan, shards, seqs, dev):
    buf = _fill(plan, seqs, dev)
    return [buf[s.info.input_begin:max(s.info.input_end, s.info.input_begin + 64)].clone() for s in shards]


def _check_merge(plan, msgs, seqs, orac, ctx):
    import teloscope_amd as ta
    from teloscope_amd.distributed import finalize_shards, free_segments
    rc, out, cnt = finalize_shards(plan, msgs)
    assert rc == 0, (ctx, rc, plan.teloscope._ctx.error())
    for i, s in enumerate(seqs):
        assert_visible_view_equal(ta.SegmentData(out[i], False), orac.scan_segment(s, 0, False), False, cnt[i], "%s segment %d" % (ctx, i))
    free_segments(plan, out)


def _poison_between_shards(rng, opts, plan, lens, margin=60_000):
    """The poison, except random sequence for `margin` bases either side of every shard boundary inside a segment: a telomere
    through the boundary outruns the context tiles, which ts_shards_finalize reports (TS_SHARD_NEED_FULL) rather than
    answers — this one the shards can answer."""
    from teloscope_amd.distributed import shard_info
    seqs = [bytearray(x) for x in _poison(rng, opts, lens)]
    tiles = plan.tiles
    for p in range(1, plan.world):
        t = int(shard_info(plan, p).own_begin)
        si, at = int(tiles["seg_index"][t]), int(tiles["seg_offset"][t])
        a, b = max(0, at - margin), min(lens[si], at + margin)
        seqs[si][a:b] = seqgen.random_dna(rng, b - a).tobytes()
    return [bytes(x) for x in seqs]


def _settle_scale(shards, loc, sptr):
    """Packs one input unpipelined until it fits (sync on a scan overflow, a larger scale on a message overflow)."""
    from teloscope_amd import _capi as K
    for _ in range(6):
        grow = 1
        for s, lo in zip(shards, loc):
            for _ in range(4):
                s.scan_pack(lo.data_ptr(), sptr, 0)
                st = s.status(0)
                if not (st.flags & K.SHARD_OVERFLOW_SCAN):
                    break
                s.sync(0)
            if st.flags & (K.SHARD_OVERFLOW_VISIBLE | K.SHARD_OVERFLOW_BLOCKS):
                grow = max(grow, 2, int(st.scale_factor_needed))
        if grow == 1:
            return
        for s in shards:
            s.set_scale(s.scale * grow)
    raise AssertionError("the poison's message kept overflowing")


@pytest.mark.parametrize("bind", ["1", "0"], ids=["bound", "unbound"])
def test_shard_slots_pipelined_with_changing_input(bind, monkeypatch):
    """Two parts, three slots each, six steps of new input (one the poison), pipelined as the bench pipelines them: step i+1's
    scan is enqueued before step i's message is read; each slot's reader is handed to PackedShard.release.  Every step's
    merged messages equal the oracle for that step's input — with bound messages and with TS_SHARD_BIND=0."""
    import torch
    from teloscope_amd import _capi as K
    from teloscope_amd import distributed as D
    monkeypatch.setenv("TS_SHARD_BIND", bind)
    lens = [900_001, 250_003, 0, 77_777, 333]
    slots = 3
    dev, opts, tel, plan, shards = _shard_setup(HEADLINE, lens, slots)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(31)
    inputs = [_sparse(rng, opts, lens) for _ in range(6)]
    inputs[2] = _poison_between_shards(rng, opts, plan, lens)
    scan_s, pack_s, read_s = D.concurrent_streams(tel, dev, 3)
    _settle_scale(shards, _locals(plan, shards, inputs[2], dev), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    pending, keep = {}, []

    def enqueue(i):
        j = i % slots
        loc = _locals(plan, shards, inputs[i], dev)
        keep.append(loc)                                      # (read on other streams: alive until the end)
        scan_s.wait_stream(torch.cuda.current_stream())       # the bytes were written on the current stream
        snaps, evs = [], []
        for s, lo in zip(shards, loc):
            s.scan(lo.data_ptr(), C.c_void_p(scan_s.cuda_stream), j)
            with torch.cuda.stream(pack_s):
                s.wait_scan(C.c_void_p(pack_s.cuda_stream), j)
                s.pack(C.c_void_p(pack_s.cuda_stream), j)
                packed = torch.cuda.Event()
                packed.record(pack_s)
            with torch.cuda.stream(read_s):                   # the "transfer": a copy of the message on a stream of its own
                read_s.wait_event(packed)
                snaps.append(s.msgs[j].clone())
                ev = torch.cuda.Event()
                ev.record(read_s)
            s.release(j, ev)
            evs.append(ev)
        pending[i] = (loc, snaps, evs)

    def read(i):
        loc, snaps, evs = pending.pop(i)
        for ev in evs:
            ev.synchronize()
        msgs = [m.cpu().numpy() for m in snaps]
        j = i % slots
        redo = False
        for p, (s, m) in enumerate(zip(shards, msgs)):
            st = K.ShardStatus()
            assert plan.L.ts_shard_peek(m.ctypes.data, m.nbytes, C.byref(st)) == 0
            assert not (st.flags & (K.SHARD_OVERFLOW_VISIBLE | K.SHARD_OVERFLOW_BLOCKS)), (i, p, hex(st.flags))
            if st.flags & K.SHARD_OVERFLOW_SCAN:              # recovered as the bench's check does: sync, then scan + pack again
                torch.cuda.synchronize()
                s.sync(j)
                s.scan_pack(loc[p].data_ptr(), C.c_void_p(scan_s.cuda_stream), j)
                torch.cuda.synchronize()
                msgs[p] = s.msgs[j].cpu().numpy()
                redo = True
        _check_merge(plan, msgs, inputs[i], orac, "step %d%s (bind %s)" % (i, " after sync" if redo else "", bind))

    for i in range(len(inputs)):
        enqueue(i)
        if i:
            read(i - 1)
    read(len(inputs) - 1)
    torch.cuda.synchronize()
    for s in shards:
        s.close()
    plan.close()


def test_visible_record_overflow_then_clean_step(monkeypatch):
    """TS_VIS_CAP=64: a telomere-rich step overflows the visible-record regions (TS_SHARD_F_SCAN_OVERFLOW in the header), sync
    regrows and rescans, the merge equals the oracle; the next step, new and sparse, carries no overflow flag and merges to
    the oracle too."""
    import torch
    from teloscope_amd import _capi as K
    monkeypatch.setenv("TS_VIS_CAP", "64")
    lens = [900_000, 250_003]
    dev, opts, tel, plan, shards = _shard_setup(HEADLINE + " -t 3000", lens, 1)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(3)
    rich = [seqgen.chromosome(rng, n, opts.canonical_fwd, opts.canonical_rev, telo_repeats=1500, n_its=5) for n in lens]
    clean = _sparse(rng, opts, lens)
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    syncs = 0
    for name, seqs in (("telomere-rich", rich), ("clean", clean)):
        msgs = []
        for s, lo in zip(shards, _locals(plan, shards, seqs, dev)):
            s.scan_pack(lo.data_ptr(), sptr, 0)
            st = s.status(0)
            if name == "clean":
                assert st.flags == 0, hex(st.flags)
            elif st.flags & K.SHARD_OVERFLOW_SCAN:
                s.sync(0)
                syncs += 1
                s.scan_pack(lo.data_ptr(), sptr, 0)
                assert not (s.status(0).flags & K.SHARD_OVERFLOW_SCAN)
            msgs.append(s.msgs[0].cpu().numpy().copy())
        _check_merge(plan, msgs, seqs, orac, name)
    assert syncs >= 1, "a 64-record region did not overflow on a telomere: the path under test did not run"
    for s in shards:
        s.close()
    plan.close()


# ------------------------------------------------------------------------------------------------------------------- E
def test_bound_message_is_not_overwritten_while_it_is_read():
    """The transfer of a slot's message held back on purpose: a reader stream waits for step 0's pack, spins (torch.cuda._sleep)
    and only then copies the message.  Meanwhile step 1 (other slot) and step 2 (the same slot, other input) are enqueued.
    With the reader handed to PackedShard.release, step 2's scan waits for it: the copy is step 0's message — byte for byte
    what an unpipelined scan + pack of step 0's input gives (blocks as a set: the kernels append them in completion order),
    and merged with the other part it equals the oracle for step 0.  Ordered behind the pack alone, step 2's scan writes its
    window records into the message under the reader."""
    import torch
    from tests import shardpack
    from teloscope_amd import distributed as D
    lens = [700_001, 250_003, 60_000]
    slots = 2
    dev, opts, tel, plan, shards = _shard_setup(HEADLINE, lens, slots)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(47)
    inputs = [_sparse(rng, opts, lens) for _ in range(3)]
    locs = [_locals(plan, shards, x, dev) for x in inputs]
    scan_s, read_s = D.concurrent_streams(tel, dev, 2)
    sptr = C.c_void_p(scan_s.cuda_stream)
    torch.cuda.synchronize()
    snaps, t0, t1 = [], torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for p, s in enumerate(shards):
        s.scan_pack(locs[0][p].data_ptr(), sptr, 0)
        packed = torch.cuda.Event()
        packed.record(scan_s)
        with torch.cuda.stream(read_s):
            read_s.wait_event(packed)
            if p == 0:
                t0.record(read_s)
                torch.cuda._sleep(40_000_000)                  # ~10-20 ms of clock: bounded, not a hang
                t1.record(read_s)
            snaps.append(s.msgs[0].clone())
            ev = torch.cuda.Event()
            ev.record(read_s)
        s.release(0, ev)
    for i in (1, 2):
        for p, s in enumerate(shards):
            s.scan_pack(locs[i][p].data_ptr(), sptr, i % slots)
    torch.cuda.synchronize()
    spin_ms = t0.elapsed_time(t1)
    print("reader held the message back for %.1f ms" % spin_ms)
    assert spin_ms > 2.0, "the reader's spin was too short to hold the transfer back (%.2f ms)" % spin_ms
    got = [m.cpu().numpy() for m in snaps]
    # the unpipelined witness: one scan + pack of step 0's input on fresh single-slot shards
    alone = [D.PackedShard(plan, p, dev, slots=1) for p in range(plan.world)]
    want = []
    for p, s in enumerate(alone):
        s.scan_pack(locs[0][p].data_ptr(), sptr, 0)
        torch.cuda.synchronize()
        want.append(s.msgs[0].cpu().numpy())
    for p in range(plan.world):
        hg, hw = shardpack.read_header(got[p]), shardpack.read_header(want[p])
        assert hg == hw, (p, hg, hw)
        nseg, nown, nwin = int(hg["n_segs"]), int(hg["own_end"] - hg["own_begin"]), int(hg["n_windows"])
        off = shardpack.sections(D.shard_info(plan, p), nseg, nown, nwin)
        assert np.array_equal(got[p][128:off["blocks"]], want[p][128:off["blocks"]]), \
            "part %d: the message read is not step 0's (window records of another step)" % p
        nb = int(hg["n_blocks"])
        key = ("seg", "kind", "seq", "start")
        bg = np.frombuffer(got[p][off["blocks"]:off["blocks"] + nb * 64].tobytes(), dtype=shardpack.DEVBLOCK_DT)
        bw = np.frombuffer(want[p][off["blocks"]:off["blocks"] + nb * 64].tobytes(), dtype=shardpack.DEVBLOCK_DT)
        assert np.array_equal(np.sort(bg, order=key), np.sort(bw, order=key)), p
    _check_merge(plan, got, inputs[0], orac, "step 0 read behind a held-back transfer")
    for s in shards + alone:
        s.close()
    plan.close()
