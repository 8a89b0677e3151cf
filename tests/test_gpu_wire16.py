"""GPU: the full exchange's u16 wire (teloscope_amd.distributed.gather_shards, the path TS_SHARD_NEED_FULL sends callers to).

ts_batch_wire16_ok promises that every u32 of a rank's three result arrays — window records, tile directory entries, the
tile-ordered match records — fits 16 bits; gather_shards then narrows them (`.to(torch.int16)`) and ts_widen_u16
(exchange.hip: an aligned 16-byte path and an element-wise one, chosen by pointer alignment) widens them where they land.
Here: the kernel at every length and alignment against `src.to(int32) & 0xFFFF`; the promise against what the scan kernels
really leave, up to the edge (a window field of 65502 at w = 10922); and the narrowed arrays of real scans, widened into an
assembly at the offsets gather_shards computes, against the oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import shardwidths
from tests.backends import BLOCK_FIELDS, assert_segment_equal, segment_as_dict

pytestmark = pytest.mark.gpu
HEADLINE = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -m -i"
SENTINEL = 0x5A5A5A5A


def _teloscope(cli, device=0):
    import teloscope_amd as ta
    from teloscope_amd.cli import parse_cli, user_input
    opts = parse_cli("x.fa " + cli)
    return opts, ta.Teloscope(user_input(opts, device=device))


def test_widen_u16_every_length_and_alignment():
    """ts_wire_widen_u16, directly and through distributed._widen_u16: lengths around the 8-element lane, the 2048-element
    workgroup and beyond; the source at every 2-byte phase of a 16-byte row, the destination at every 4-byte phase; 0x0000,
    0x7FFF, 0x8000 and 0xFFFF at both ends (a sign-extending widen turns the last two into 0xFFFF8000 and 0xFFFFFFFF) and
    random values between; 64 sentinels either side of the destination stay what they were."""
    import torch
    from teloscope_amd import _capi as K
    from teloscope_amd import distributed as D
    dev = torch.device("cuda", 0)
    opts, tel = _teloscope(HEADLINE)
    plan = D.ShardPlan(tel, [5000], world=1)
    L = K.lib()
    rng = np.random.default_rng(16)
    edges = np.array([0x0000, 0x7FFF, 0x8000, 0xFFFF] * 2, dtype=np.uint16)
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4097):
        vals = rng.integers(0, 65536, size=n, dtype=np.uint16)
        m = min(8, n)
        vals[:m] = edges[:m]
        vals[n - m:] = edges[::-1][:m]
        if n >= 8:
            assert {0x0000, 0x7FFF, 0x8000, 0xFFFF} <= set(vals[:8].tolist()) and {0x0000, 0x7FFF, 0x8000, 0xFFFF} <= set(vals[-8:].tolist())
        host = torch.from_numpy(vals.view(np.int16).copy()).to(dev)
        for so in range(8):
            src_buf = torch.zeros(n + 16, dtype=torch.int16, device=dev)
            assert src_buf.data_ptr() % 16 == 0
            src = src_buf[so:so + n]
            src.copy_(host)
            for do in range(4):
                want = torch.full((64 + do + n + 64,), SENTINEL, dtype=torch.int32, device=dev)
                assert want.data_ptr() % 16 == 0
                want[64 + do:64 + do + n] = src.to(torch.int32) & 0xFFFF
                for call in ("capi", "distributed"):
                    dst_buf = torch.full((64 + do + n + 64,), SENTINEL, dtype=torch.int32, device=dev)
                    dst = dst_buf[64 + do:64 + do + n]
                    if call == "capi":
                        rc = L.ts_wire_widen_u16(tel._ctx.ptr, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
                        assert rc == 0, tel._ctx.error()
                    else:
                        D._widen_u16(plan, src, dst)
                    if not torch.equal(dst_buf, want):
                        bad = torch.nonzero(dst_buf != want).flatten()[:8].tolist()
                        raise AssertionError("n %d, source element offset %d, destination element offset %d (%s): differs at %s (the destination is [%d, %d))"
                                             % (n, so, do, call, bad, 64 + do, 64 + do + n))
    plan.close()


WIRE_CASES = [(shardwidths.cli(e), e) for e in shardwidths.WIDTH_GRID] + [(HEADLINE, None), ("-t 3000", None)]


@pytest.mark.parametrize("cli,entry", WIRE_CASES, ids=[shardwidths.entry_id(e) if e else c for c, e in WIRE_CASES])
def test_wire16_ok_is_true_only_where_every_value_fits(cli, entry):
    """Wherever a plan says its arrays may travel as u16, the largest value the scan kernels leave in them — window records,
    tile directory entries, match records, of the grid's homopolymer and chromosome — must fit 16 bits: the gather would
    truncate it silently.  The grid reaches the promise's edge from both sides: w = 10922 may (k x w = 65532, a window field
    of 65502), w = 10923 may not (k x w = 65538), and w = 16384 may not because a tile outgrows the records' 14-bit positions."""
    import torch
    from teloscope_amd.distributed import ShardPlan
    dev = torch.device("cuda", 0)
    opts, tel = _teloscope(cli)
    seqs, abs_pos = shardwidths.inputs(opts)
    plan = ShardPlan(tel, [len(s) for s in seqs], abs_pos=abs_pos, tips_only=opts.ultra_fast, world=2)
    parts, counts = shardwidths.scan_parts(plan, shardwidths.fill(plan, seqs, dev), dev)
    assert sum(counts) > 0
    u32max = lambda t: int(t.to(torch.int64).bitwise_and(0xFFFFFFFF).max()) if t.numel() else 0
    top = {name: max(u32max(p[i]) for p in parts) for i, name in enumerate(("windows", "stats", "dense"))}
    if plan.wire16_ok:
        assert max(top.values()) <= 65535, (cli, top)
    w = entry[0] if entry else None
    if entry == (10922, 5461, "-r -g"):
        assert plan.wire16_ok and 65500 <= top["windows"] <= 65535, top          # 10917 matches x 6 = 65502
    if entry == (10923, 10923, "-r -g"):
        assert 6 * w > 65535 and not plan.wire16_ok
    if entry == (16384, 16384, "-r -g"):
        assert int(plan.tiles["owned_bases"].max()) + 64 > 1 << 14 and not plan.wire16_ok
    if entry is None:
        assert plan.wire16_ok                                   # (the sets the bench and the gloo tests send as u16)
    plan.close()


@pytest.mark.parametrize("cli", [HEADLINE, shardwidths.cli((10922, 5461, "-r -g")), shardwidths.cli((511, 511, "-r -g")), "-t 3000"],
                         ids=["headline", "w10922-s5461", "w511-s511", "tips"])
def test_full_exchange_over_the_u16_wire_equals_the_oracle(cli):
    """What gather_shards does on the destination, without the ranks: every part's arrays narrowed as they are for the wire
    (`.to(torch.int16)`), landed in a buffer shaped like the gather's, and widened by distributed._widen_u16 into slices of one
    Assembled at the offsets the gather computes — 8 x window_begin, 4 x tile_begin and the running record count, which is
    arbitrary, so that the element-wise path runs on real data.  The assembly must be the un-narrowed concatenation bit for
    bit, and adopted (ts_batch_adopt) it must download to the oracle's segments and blocks."""
    import torch
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.distributed import Assembled, ShardPlan, _widen_u16, adopt
    dev = torch.device("cuda", 0)
    L = K.lib()
    opts, seqs, abs_pos, exp = shardwidths.reference(cli)
    _, tel = _teloscope(cli)
    tips = opts.ultra_fast
    lens = [len(s) for s in seqs]
    unaligned = 0
    for world in (2, 3):
        plan = ShardPlan(tel, lens, abs_pos=abs_pos, tips_only=tips, world=world)
        assert plan.wire16_ok
        parts, counts = shardwidths.scan_parts(plan, shardwidths.fill(plan, seqs, dev), dev)
        total = sum(counts)
        a = Assembled(torch.full((8 * plan.n_windows,), SENTINEL, dtype=torch.int32, device=dev),
                      torch.full((4 * plan.n_tiles,), SENTINEL, dtype=torch.int32, device=dev),
                      torch.full((max(total, 1),), SENTINEL, dtype=torch.int32, device=dev), total, counts)
        rec_off = np.concatenate(([0], np.cumsum(counts))).tolist()
        for p in range(world):
            rp = plan.ranges[p]
            slots = (a.windows[8 * rp.window_begin:8 * rp.window_end] if not tips else a.windows[:0],
                     a.stats[4 * rp.tile_begin:4 * rp.tile_end], a.dense[rec_off[p]:rec_off[p + 1]])
            for t, full in zip(slots, parts[p]):
                assert t.numel() == full.numel()
                if not t.numel():
                    continue
                tmp = torch.empty(t.numel() + t.numel() // 8 + 16, dtype=torch.int16, device=dev)[:t.numel()]
                tmp.copy_(full.to(torch.int16))                  # keeps the low 16 bits: what travels
                unaligned += int(t.data_ptr() % 16 != 0)
                _widen_u16(plan, tmp, t)
        for i, name in enumerate(("windows", "stats", "dense")):
            whole = torch.cat([p[i] for p in parts])
            assert torch.equal(getattr(a, name)[:whole.numel()], whole), (cli, world, name)
        b = adopt(plan, a)
        out = (K.SegmentOut * len(lens))()
        assert L.ts_batch_download(b, None, out) == 0, tel._ctx.error()
        for i in range(len(lens)):
            assert_segment_equal(segment_as_dict(ta.SegmentData(out[i], tips)), exp[i], tips, ctx="%s world %d segment %d" % (cli, world, i))
        L.ts_free_segments(out, len(lens))
        out2 = (K.SegmentOut * len(lens))()
        assert L.ts_batch_download_blocks(b, out2) == 0, tel._ctx.error()
        for i in range(len(lens)):
            g = ta.SegmentData(out2[i], tips)
            for f in BLOCK_FIELDS:
                assert np.array_equal(g.terminalBlocks[f], exp[i]["terminal_blocks"][f]), (cli, world, i, f)
                assert np.array_equal(g.interstitialBlocks[f], exp[i]["interstitial_blocks"][f]), (cli, world, i, f)
        L.ts_free_segments(out2, len(lens))
        L.ts_batch_destroy(b)
        plan.close()
    # (a tips-only plan is cut at segment starts, and the run of A holds no match of its patterns: its parts land at record 0)
    assert tips or unaligned > 0, "every destination was 16-byte aligned: the element-wise path did not run on real data"
