"""Device block calling at its exact thresholds (the hand-built cases of tests/blockcases.py, which
tests/test_oracle_block_thresholds.py pins on the oracle) through every route that can take them, record for record
against the oracle.  Each case also runs moved so that the two matches that decide it straddle a tile boundary of the
tiled kernel (read from the plan), a tile of the general kernels (TS_GENERAL_TILE positions from the region start, the
constant read from the library header), record 63/64/65 of a wave walk (asserted from the plan), and the
part boundary of a two- and a three-part ts_scan_segments_multi split; every straddle is asserted, not assumed."""
import ctypes as C

import numpy as np
import pytest

from tests import blockcases as BC
from tests import harness as H
from tests.backends import (BLOCK_FIELDS, OracleBackend, OracleReadFilter, ProductBackend, ProductReadFilter,
                            assert_segment_equal, assert_visible_view_equal)

pytestmark = pytest.mark.gpu

def _general_tile():
    """TS_GENERAL_TILE, read from the library's header: the general kernels tile a scanned region from its start"""
    import os
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "teloscope_amd", "csrc", "ts_internal.h")
    return int(re.search(r"#define TS_GENERAL_TILE (\d+)", open(hdr).read()).group(1))


GENERAL_TILE = _general_tile()
T_MOVED = 1_000_000                  # moved terminal cases: the whole segment is terminal zone (the zone has cases of its own)


def _tiles(ctx_ptr, n, tips):
    """[(first, end)) of the owned bases of every tile of a one-segment plan (ts_batch_get_tiles)"""
    from teloscope_amd import _capi as K
    L = K.lib()
    lens = (C.c_uint64 * 1)(n)
    b = L.ts_batch_create(ctx_ptr, lens, None, 1, int(tips), 0)
    assert b, L.ts_last_error(ctx_ptr)
    try:
        info = K.BatchInfo()
        L.ts_batch_get_info(b, C.byref(info))
        arr = (K.TileInfo * max(1, info.n_tiles))()
        assert L.ts_batch_get_tiles(b, 0, info.n_tiles, arr) == 0
        return [(arr[t].seg_offset, arr[t].seg_offset + arr[t].owned_bases) for t in range(info.n_tiles)]
    finally:
        L.ts_batch_destroy(b)


def _plan_tiles(cmd, n, tips, world=1):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    from teloscope_amd.distributed import ShardPlan
    tel = ta.Teloscope(user_input(H.parse_cli(cmd), device=K.DEVICE_NONE))           # planning only
    plan = ShardPlan(tel, [n], abs_pos=[0], tips_only=tips, world=world)
    offs = [int(x) for x in plan.tiles["seg_offset"]]
    parts = [offs[r.tile_begin] for r in plan.ranges[1:] if 0 < r.tile_begin < len(offs)]
    return offs, parts


def _general_tiles(n):
    return [(a, min(n, a + GENERAL_TILE)) for a in range(0, n, GENERAL_TILE)]


def _walk_index(positions, tiles, pos, from_end):
    """(tile, index of the record at `pos` among its tile's records in walk order: from the tile's first record, or from
    its last for a walk from the end)"""
    for t, (a, b) in enumerate(tiles):
        if a <= pos < b:
            recs = [p for p in positions if a <= p < b]
            k = recs.index(pos)
            return t, (len(recs) - 1 - k if from_end else k)
    raise AssertionError("position %d lies in no tile" % pos)


def assert_at_step(positions, tiles, first, second, index, from_end, what):
    """the pair (first, second in walk order) lies in one tile with `second` at record `index` of that tile's walk; at
    index 64 the two lie on both sides of a 64-record step"""
    t1, k1 = _walk_index(positions, tiles, first, from_end)
    t2, k2 = _walk_index(positions, tiles, second, from_end)
    assert t1 == t2 and k2 == index and k1 == index - 1, "%s: pair at tile %d record %d / tile %d record %d, not %d" % (
        what, t1, k1, t2, k2, index)
    assert (k1 // 64 != k2 // 64) == (index == 64), what


def _positions(lay, cmd, tips):
    e = OracleBackend(H.parse_cli(cmd)).scan_segment(lay.seq(), 0, tips)
    return sorted({int(p) for name in ("fwd_matches", "rev_matches") for p in e[name]["position"]})


def placements(case):
    """[(placement name, Layout, t)] for one case; every straddle is asserted from a plan's tiles"""
    out = [("as built", case.layout, case.t)]
    if not case.pair:
        return out
    a, b = case.deciding_positions()
    tips = not case.full
    t_moved = T_MOVED if case.side in ("p", "q") else case.t
    tiled = "-p " not in case.cli               # a mixed-length set has no tiled plan (the general kernels take it)
    from_end = case.side == "q"
    for idx in (63, 64, 65):
        v = BC.at_record_index(case.layout, case.pair, idx, case.side, BC.filler_spacing(case.cli, case.full))
        if not v:
            continue
        lay, shift = v
        cmd = case.command(t_moved)
        pos = _positions(lay, cmd, tips)
        first, second = (b + shift, a + shift) if from_end else (a + shift, b + shift)
        where = "%s record %d" % (case.name, idx)
        if tiled:
            assert_at_step(pos, _tiles(_plan_ctx(cmd), lay.n, tips), first, second, idx, from_end, where + " (tiled plan)")
        assert_at_step(pos, _general_tiles(lay.n), first, second, idx, from_end, where + " (general tiles)")
        out.append(("record %d of its tile's walk %s" % (idx, "from the end" if from_end else "from the start"), lay, t_moved))
    # a tile boundary of the tiled kernel: background in front puts match j on it (the q side keeps its distance to the end)
    if tiled:
        offs, _ = _plan_tiles(case.command(t_moved), case.layout.n + 40000, tips)
        bound = next((o for o in offs if o > b + 200), None)
        assert bound is not None, case.name
        pad = bound - b
        lay = case.layout.shifted(pad)
        offs, _ = _plan_tiles(case.command(t_moved), lay.n, tips)
        assert any(a + pad < o <= b + pad for o in offs), "%s: no tile boundary of the plan between the pair" % case.name
        out.append(("tiled-kernel tile boundary at %d" % bound, lay, t_moved))
    # a tile of the general kernels: one scanned region from position 0 (full scan, or n <= 2t)
    pad = 2 * GENERAL_TILE - b
    lay = case.layout.shifted(pad)
    assert case.full or lay.n <= 2 * t_moved, case.name
    out.append(("general-kernel tile boundary at %d" % (2 * GENERAL_TILE), lay, t_moved))
    return out


_PLAN_CTX = {}


def _plan_ctx(cmd, read_filter=False):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    key = (cmd, read_filter)
    if key not in _PLAN_CTX:
        ui = user_input(H.parse_cli(cmd), device=K.DEVICE_NONE)
        _PLAN_CTX[key] = ta.ReadTelomereFilter(ui) if read_filter else ta.Teloscope(ui)
    return _PLAN_CTX[key]._ctx.ptr


def multi_placements(case, world):
    """the deciding pair across the part boundary of a `world`-part split of one segment of fixed length"""
    N = 200000                           # (a split keeps clear of segment ends)
    cmd = case.command()
    a, b = case.deciding_positions()
    _, parts = _plan_tiles(cmd, N, False, world)
    assert parts, "%s: a %d-part split of %d bases has no inner boundary" % (case.name, world, N)
    bound = parts[0]
    pad = bound - b
    assert pad >= 0
    lay = case.layout.shifted(pad, tail=N - case.layout.n - pad)
    _, parts = _plan_tiles(cmd, lay.n, False, world)
    assert any(a + pad < p <= b + pad for p in parts), "%s: part boundary not straddled" % case.name
    return lay, cmd, bound


def _by_command(cases):
    groups = {}
    for c in cases:
        for name, lay, t in placements(c):
            groups.setdefault(c.command(t), []).append((c, name, lay))
    return groups


def _check(prod_out, orac, items, tips, route):
    for (case, name, lay), g in zip(items, prod_out):
        e = orac.scan_segment(lay.seq(), 0, tips)
        assert_segment_equal(g, e, tips, ctx="case %s route %s placement %s:" % (case.name, route, name))


ROUTED = BC.ALL_CASES
GROUPS = _by_command(ROUTED)
CMDS = sorted(GROUPS)


def _scan(opts, items, tips, route, monkeypatch, env=()):
    for k, v in env:
        monkeypatch.setenv(k, v)
    try:
        prod = ProductBackend(opts)
        got = prod.scan_segments([(lay.seq(), 0, tips) for _, _, lay in items])
    finally:
        for k, _ in env:
            monkeypatch.delenv(k, raising=False)
    return prod, got


def _record_bits(prod, items, tips):
    """the record width of the context's batches: a scanned batch of 32-bit records gives a raw view of them
    (ts_batch_matches_ptr), one of 16-bit records does not"""
    from teloscope_amd import _capi as K
    L = K.lib()
    seqs = [lay.seq() for _, _, lay in items]
    lens = (C.c_uint64 * len(seqs))(*[len(x) for x in seqs])
    ctx = prod.teloscope._ctx.ptr
    b = L.ts_batch_create(ctx, lens, None, len(seqs), int(tips), 0)
    assert b, L.ts_last_error(ctx)
    try:
        for i, x in enumerate(seqs):
            assert L.ts_batch_upload(b, i, x) == 0
        assert L.ts_batch_scan(b, None, None) == 0 and L.ts_batch_sync(b) == 0, L.ts_last_error(ctx)
        return 32 if L.ts_batch_matches_ptr(b) else 16
    finally:
        L.ts_batch_destroy(b)


def _blocks_only(prod, orac, items, tips, route):
    bl, counts = prod.teloscope.scanSegmentsBlocksOnly([(lay.seq(), 0) for _, _, lay in items], tipsOnly=tips, with_counts=True)
    for (case, name, lay), g, cnt in zip(items, bl, counts):
        e = orac.scan_segment(lay.seq(), 0, tips)
        ctx = "case %s route %s placement %s" % (case.name, route, name)
        assert cnt[1] == len(e["fwd_matches"]) + len(e["rev_matches"]) and cnt[3] == len(e["fwd_matches"]), ctx
        for nm, gb in (("terminal_blocks", g.terminalBlocks), ("interstitial_blocks", g.interstitialBlocks)):
            assert len(gb) == len(e[nm]), "%s %s count" % (ctx, nm)
            for f in BLOCK_FIELDS:
                assert np.array_equal(gb[f], e[nm][f]), "%s %s.%s" % (ctx, nm, f)


@pytest.mark.parametrize("cmd", CMDS)
def test_cases_through_every_route(cmd, monkeypatch, capfd):
    import re
    items = GROUPS[cmd]
    opts = H.parse_cli(cmd)
    tips = opts.ultra_fast
    orac = OracleBackend(opts)
    default_set = "-p " not in cmd
    # the default route (the tiled kernel for the default pattern set) with 16-bit records, then with 32-bit records;
    # full results and blocks only on each
    for route, env, bits in (("default", [], 16), ("TS_REC32=1", [("TS_REC32", "1")], 32)):
        prod, got = _scan(opts, items, tips, route, monkeypatch, env)
        tiled = prod.teloscope.usesFastPath()
        assert tiled or not default_set, cmd
        route += " (tiled)" if tiled else " (general)"
        if tiled:
            assert _record_bits(prod, items, tips) == bits, route
        _check(got, orac, items, tips, route)
        _blocks_only(prod, orac, items, tips, route + " blocks-only")
    # the general kernels: the list form of the fused pass, and the position-strided form (TS_GEN_LIST=0); the library
    # says under TS_TIMING how many groups took each
    for route, env, form in (("general list form", [("TS_FORCE_GENERAL", "1"), ("TS_TIMING", "1")], 0),
                             ("general strided form", [("TS_FORCE_GENERAL", "1"), ("TS_GEN_LIST", "0"), ("TS_TIMING", "1")], 1)):
        capfd.readouterr()
        prod, got = _scan(opts, items, tips, route, monkeypatch, env)
        err = capfd.readouterr().err
        assert not prod.teloscope.usesFastPath(), route
        assert "route: table form, blocks called on the device" in err, (route, err[-2000:])
        forms = re.findall(r"fused pass: (\d+) groups in the list form, (\d+) in the strided form", err)
        assert forms and all(int(f[form]) > 0 and int(f[1 - form]) == 0 for f in forms), (route, forms)
        _check(got, orac, items, tips, route)


def _with_patterns(cmd, extra):
    opts = H.parse_cli(cmd)
    pats = list(opts.raw_patterns) + [extra]
    toks = cmd.split()
    if "-p" in toks:
        k = toks.index("-p")
        del toks[k:k + 2]
    return " ".join(toks) + " -p " + ",".join(pats)


@pytest.mark.parametrize("cmd", CMDS)
def test_cases_through_the_wide_and_push_ordered_forms(cmd, monkeypatch, capfd):
    items = GROUPS[cmd]
    tips = H.parse_cli(cmd).ultra_fast
    forms = [("wide form", _with_patterns(cmd, BC.WIDE), "route: wide form")]
    if not tips:                         # push order: pattern lengths 6 and 9 under w > s
        forms.append(("push-ordered stream", _with_patterns(cmd, "GATTACAGA") + " -w 200 -s 100", "written in push order"))
    for route, c2, needle in forms:
        opts = H.parse_cli(c2)
        orac = OracleBackend(opts)
        capfd.readouterr()
        prod, got = _scan(opts, items, tips, route, monkeypatch, [("TS_TIMING", "1")])
        err = capfd.readouterr().err
        assert not prod.teloscope.usesFastPath() and needle in err, (route, err[-2000:])
        if orac.ambiguous:
            orac = orac.with_ambiguous_orientation_from(prod.patterns)
        _check(got, orac, items, tips, route)


TERMINAL_CMDS = sorted(c for c in CMDS if H.parse_cli(c).ultra_fast)


def per_side(blocks, n):
    best = [0, 0]
    for b in blocks:
        rel, ln = int(b["start"]), int(b["block_len"])
        best[0 if rel <= n - (rel + ln) else 1] = max(best[0 if rel <= n - (rel + ln) else 1], ln)
    return best


@pytest.mark.parametrize("cmd", TERMINAL_CMDS)
def test_terminal_ends_of_the_cases(cmd):
    """ts_terminal_ends (GFA mode): the longest block per side, a tie going to the start side"""
    items = GROUPS[cmd]
    opts = H.parse_cli(cmd)
    ends = ProductBackend(opts).teloscope.terminalEnds([lay.seq() for _, _, lay in items])
    orac = OracleBackend(opts)
    for (case, name, lay), got in zip(items, ends):
        want = per_side(orac.scan_segment(lay.seq(), 0, True)["terminal_blocks"], lay.n)
        assert list(map(int, got)) == want, "case %s route terminalEnds placement %s" % (case.name, name)
        if name == "as built" and case.name in BC.ENDS:
            assert tuple(want) == BC.ENDS[case.name], case.name


# (a split keeps each terminal zone within one part, so only the interstitial walk can have its deciding pair cut by one)
MULTI_CASES = [c for c in ROUTED if c.pair and c.side == "its" and "-p " not in c.cli]


@pytest.mark.parametrize("world", [2, 3])
def test_cases_across_the_parts_of_a_multi_context_scan(world, monkeypatch, capfd):
    """ts_scan_segments_multi on one GPU with two and three contexts: each case's deciding pair across the first part
    boundary of the split"""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    merged, fell_back = [], []
    by_cmd = {}
    for c in MULTI_CASES:
        lay, cmd, bound = multi_placements(c, world)
        by_cmd.setdefault(cmd, []).append((c, lay, bound))
    for cmd, items in sorted(by_cmd.items()):
        opts = H.parse_cli(cmd)
        tips = opts.ultra_fast
        monkeypatch.setenv("TS_TIMING", "1")               # (the contexts read it when they are made)
        tels = [ta.Teloscope(user_input(opts, device=0)) for _ in range(world)]
        monkeypatch.delenv("TS_TIMING")
        orac = OracleBackend(opts)
        for case, lay, bound in items:                       # one segment per call: the split is of that segment
            s = lay.seq()
            segs = (K.SegmentIn * 1)()
            segs[0].seq, segs[0].len, segs[0].abs_pos, segs[0].tips_only = s, len(s), 0, int(tips)
            out, cnt = (K.SegmentOut * 1)(), (K.SegmentCounts * 1)()
            ctxs = (C.c_void_p * world)(*[t._ctx.ptr for t in tels])
            capfd.readouterr()
            assert K.lib().ts_scan_segments_multi(ctxs, world, segs, 1, out, cnt) == 0, tels[0]._ctx.error()
            err = capfd.readouterr().err
            if "multi: %d shards merged" % world in err:
                merged.append(case.name)
            else:                                            # the library's documented fall-back (multi.cpp): say which
                assert "scanned again on one context" in err, (case.name, err[-2000:])
                fell_back.append(case.name)
            try:
                assert_visible_view_equal(ta.SegmentData(out[0], tips), orac.scan_segment(s, 0, tips), tips, cnt[0],
                                          "case %s route multi-%d placement part boundary at %d" % (case.name, world, bound))
            finally:
                K.lib().ts_free_segments(out, 1)
    # most placements must have been merged from the shards; the ones the library scanned again on one context are named
    assert len(merged) > len(fell_back), "multi-%d: merged %s, scanned again on one context %s" % (world, merged, fell_back)
    if fell_back:
        import warnings
        warnings.warn("multi-%d: scanned again on one context: %s" % (world, fell_back))


def _read_batch(cli):
    """every read case as built, reverse-complemented, and with its deciding pair at record 63 / 64 / 65 of the read's
    record stream, forward and reverse (pred_scan_wave walks both lists from a tile's first record), asserted from the
    read filter's plan; each long read sits among 63 short ones (see _assert_long)"""
    reads, want, names, long_ix = [], [], [], []
    opts_cmd = "x.fa --fastq-subset " + cli
    for name, c, marks, passes in BC.READ_CASES:
        if c != cli:
            continue
        lay = BC.read_layout(marks)
        pair = BC.READ_PAIRS[name]
        m = len(lay.marks)
        mpair = (m - 1 - pair[1], m - 1 - pair[0])
        reads.append(lay.seq()); want.append(passes); names.append(name + " as built")
        reads.append(lay.mirrored().seq()); want.append(passes); names.append(name + " reverse complement")
        for idx in (63, 64, 65):
            for where, base, pr, motif in (("forward", lay, pair, BC.F), ("reverse", lay.mirrored(), mpair, BC.R)):
                lr, shift = BC.long_read(base, pr, idx, cli, motif)
                pos = [p for p, _ in lr.marks]
                first, second = base.marks[pr[0]][0] + shift, base.marks[pr[1]][0] + shift
                assert_at_step(pos, _tiles(_plan_ctx(opts_cmd, True), lr.n, True), first, second, idx, False,
                               "read %s %s record %d (read filter plan)" % (name, where, idx))
                reads += [(BC.BG * 100).encode()] * 63
                want += [False] * 63
                names += ["background"] * 63
                long_ix.append(len(reads))
                reads.append(lr.seq()); want.append(passes); names.append("%s %s record %d" % (name, where, idx))
    return reads, want, names, long_ix


def _assert_long(reads, long_ix, names):
    """the predicate lists a read for a whole wave when its list is above 128 records and above twice the mean of its
    wave of 64 reads (predicate.hip): true of each long read whichever 64 consecutive reads form its wave"""
    counts = [r.count(BC.F.encode()) + r.count(BC.R.encode()) + r.count(BC.FN.encode()) + r.count(BC.RN.encode()) for r in reads]
    for k in long_ix:
        assert counts[k] > 128, names[k]
        for w0 in range(max(0, k - 63), k + 1):
            win = counts[w0:w0 + 64]
            assert counts[k] > 2 * sum(win) / 64.0, names[k]


@pytest.mark.parametrize("cli", sorted({c[1] for c in BC.READ_CASES}))
def test_read_filter_cases(cli, monkeypatch):
    opts = H.parse_cli("--fastq-subset " + cli)
    reads, want, names, long_ix = _read_batch(cli)
    _assert_long(reads, long_ix, names)
    exp = OracleReadFilter(opts).filter(reads)
    assert exp == want
    for route, env in (("read filter", None), ("read filter TS_REC32=1", "1")):
        if env:
            monkeypatch.setenv("TS_REC32", env)
        got = ProductReadFilter(opts).filter(reads)
        monkeypatch.delenv("TS_REC32", raising=False)
        bad = [names[k] for k in range(len(reads)) if got[k] != exp[k]]
        assert not bad, "route %s cli %r: %s" % (route, cli, bad)
