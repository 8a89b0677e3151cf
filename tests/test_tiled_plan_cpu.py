"""The host plan of the tiled scan kernel where no device is needed.  teloscope_amd/csrc/tiled_plan_core.h — the geometry search over
the LDS layout of scan_lds_core.h, the segment loop, what a tile range covers, the terminal-zone words, the launch sizes, the
regrow rule and the shard plan, which capi.cpp and shard.cpp call — run by a program of its own under ASan + UBSan
(tests/cpp/tiled_plan_host.cpp) against the rules restated here.  And through the library: what ts_batch_get_tiles,
ts_batch_range_info, ts_batch_shard_info and ts_batch_get_info say on a planning-only context is the program's output for the
same inputs (one source: that pins the wiring only)."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
HEADER = open(os.path.join(CSRC, "ts_internal.h")).read()
CHUNK = int(re.search(r"#define TS_CHUNK\s+(\d+)", HEADER).group(1))
LIST = int(re.search(r"#define TS_LIST\s+(\d+)", HEADER).group(1))
IN_PAD = int(re.search(r"#define TS_IN_PAD\s+(\d+)", HEADER).group(1))
ZONE_NONE = int(re.search(r"#define TS_ZONE_NONE\s+(0x[0-9A-Fa-f]+)u", HEADER).group(1), 16)
CU_LDS = 160 * 1024
assert (CHUNK, LIST) == (2016, 512)


def a16(x):
    return (x + 15) & ~15


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ the inputs
def table_form(k, byte7=False):
    """(table_rows, fc_bytes, fc_byte_table, pair_byte_table) as patterns.cpp: build_match_table leaves them"""
    pair_byte = k <= 6 or (k == 7 and byte7)
    rows = 4 ** (k + 1) // (4 if pair_byte else 16)
    fc_byte = k <= 7
    fc_bytes = 0 if pair_byte else 4 * max(4 ** k // (4 if fc_byte else 16), 4)
    return rows, fc_bytes, int(fc_byte), int(pair_byte)


def inputs(s=1000, w=1000, tl=50000, k=6, npat=38, ncanon=2, nuc=1, kdist=50, byte7=False, pin=(0, 0, 0, 0), accpw=0, st32=0, viscap=0):
    rows, fcb, fc_byte, pair_byte = table_form(k, byte7)
    return SimpleNamespace(s=s, w=w, tl=tl, kdist=kdist, fold=1, nuc=nuc, k=k, npat=npat, ncanon=ncanon, rows=rows, fc_bytes=fcb,
                           fc_byte=fc_byte, pair_byte=pair_byte, pin=tuple(pin), accpw=accpw, st32=st32, viscap=viscap)


def line(i, tips):
    return " ".join(map(str, (int(tips), i.s, i.w, i.tl, i.kdist, i.fold, i.nuc, i.k, i.npat, i.ncanon, i.rows, i.fc_bytes, i.fc_byte, i.pair_byte)
                        + i.pin + (i.accpw, i.st32)))


def plan_line(i, tips, lens, cap=0, ncu=0):
    return "%s %d %d %d %d %s" % (line(i, tips), i.viscap, cap, ncu, len(lens), " ".join(map(str, lens)))


HEADLINE = dict(s=500, w=1000, npat=124)
# the six of tests/test_capi_symbols.py::test_planner_tiling_choices, with their windows per tile
KNOWN = [(inputs(**HEADLINE), 23), (inputs(s=500, w=1000, npat=2), 31), (inputs(npat=38), 16),
         (inputs(s=1000, w=2000, k=7, npat=44, byte7=True), 13), (inputs(pin=(16, 0, 0, 0), **HEADLINE), 31), (inputs(npat=38, pin=(10, 6, 0, 0)), 12)]
GEOMETRY_SETS = [(i, False) for i, _ in KNOWN] + [
    (inputs(**HEADLINE), True), (inputs(), True),                                        # tips-only
    (inputs(s=1000, w=1000, nuc=0), False),                                              # w == s
    (inputs(s=300, w=1000), False), (inputs(s=300, w=1000, nuc=0), False),               # w no multiple of s
    (inputs(s=32768, w=32768), False), (inputs(s=16384, w=32768), False),
    (inputs(s=6, w=6), False), (inputs(s=6, w=12), False), (inputs(s=3, w=3, k=3, npat=16), False),      # the smallest steps
    (inputs(s=1000, w=2000, k=7, npat=44), False), (inputs(k=7, npat=44, byte7=True), True),
    (inputs(accpw=1, **HEADLINE), False), (inputs(st32=1, **HEADLINE), False), (inputs(st32=1), True),
    (inputs(pin=(12, 6, 0, 2), **HEADLINE), False), (inputs(pin=(16, 8, 256, 0), **HEADLINE), False), (inputs(pin=(1, 1, 0, 0)), False),
] + [(inputs(s=500, w=1000, k=k, npat=4 * k), False) for k in range(3, 9)] + [(inputs(s=1000, w=2000, k=k, npat=6 * k * k, nuc=0), False) for k in range(3, 9)]


# ------------------------------------------------------------------------------------------------ the core under sanitizers
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiled_plan")
    exe = str(d / "tiled_plan_host")
    src = os.path.join(ROOT, "tests", "cpp", "tiled_plan_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        if subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, timeout=60, env=ENV).returncode == 0:
            break

    def run(cases):
        r = subprocess.run([exe], input="".join(c + "\n" for c in cases).encode(), capture_output=True, timeout=300, env=ENV)
        assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(cases)
        return lines
    return run


GEOM_FIELDS = ("wgs waves nch wpt lds stage_cap stage_u16 acc_copies div_exact s_magic22 vis_wide halo s w max_windows acc_blocks block_sums "
               "nuc_on windows_on straddle s_inv fold_mask kdist").split()


def parse_geom(text):
    head, tail = text.split(" : ")
    t = head.split()
    assert t[0] == "geom" and len(t) == 1 + len(GEOM_FIELDS), text
    g = SimpleNamespace(**dict(zip(GEOM_FIELDS, map(int, t[1:]))))
    g.codes, g.rec, g.wacc, g.stage, g.park, g.slice_bytes, g.queue = map(int, tail.split())
    return g


def geometry(host, i, tips):
    return parse_geom(host(["geom " + line(i, tips)])[0])


# ------------------------------------------------------------------------------------------------------------ geometry
def lds_of(g, i):
    """The LDS layout's sentence: [match table, up to the queues' own size][a queue per wave][a slice per wave]; a slice = codes
    | rec | wacc | stage | park"""
    codes = a16((g.nch * 63 + 1) * 8)
    rec = a16((g.max_windows + g.halo) * 16) if g.windows_on and g.nuc_on else 0
    wacc = a16((g.max_windows + (g.halo if g.acc_blocks else 0)) * 8 * (g.acc_copies + (1 if g.acc_blocks else 0))) if g.windows_on else 0
    stage = (g.stage_cap + 64) * (2 if g.stage_u16 else 4)
    offsets = (0, codes, codes + rec, codes + rec + wacc, codes + rec + wacc + stage)
    queue = cdiv(i.rows * 4 + i.fc_bytes, 2 * LIST) * 2 * LIST
    return offsets, offsets[-1] + 32, queue, queue + g.waves * (2 * LIST + offsets[-1] + 32)


def test_geometry_fits_the_lds_and_states_its_tile(host):
    lines = host(["geom " + line(i, tips) for i, tips in GEOMETRY_SETS])
    for (i, tips), text in zip(GEOMETRY_SETS, lines):
        g = parse_geom(text)
        ctx = (vars(i), tips, text)
        offsets, slice_bytes, queue, total = lds_of(g, i)
        assert (g.codes, g.rec, g.wacc, g.stage, g.park) == offsets and g.slice_bytes == slice_bytes and g.queue == queue, ctx
        assert g.lds == total and total <= CU_LDS // g.wgs, ctx
        positions = g.nch * CHUNK + 64
        assert positions <= 65535, ctx
        assert g.stage_u16 == int(positions <= 16384 and not i.st32) and g.vis_wide == int(positions > 16384), ctx
        assert g.stage_cap % 16 == 0 and g.stage_cap >= 16, ctx
        assert g.acc_copies in (1, 2, 4) and g.fold_mask == 0xDFDFDFDF and g.kdist == i.kdist, ctx
        if tips:
            assert (g.wpt, g.max_windows, g.halo, g.windows_on, g.nuc_on, g.acc_blocks, g.block_sums, g.straddle) == (1, 1, 0, 0, 0, 0, 0, 0), ctx
            assert g.s == g.w == (g.nch * CHUNK - 63) & ~15, ctx
        else:
            assert (g.s, g.w, g.halo, g.windows_on, g.nuc_on) == (i.s, i.w, cdiv(i.w, i.s) - 1, 1, i.nuc), ctx
            assert g.wpt == g.max_windows == min((g.nch * CHUNK - 63) // i.s - g.halo, 448) and g.wpt >= 1, ctx
            assert g.block_sums == int(i.w % i.s == 0) and g.acc_blocks == int(i.w % i.s == 0 and not i.accpw) and g.straddle == int(i.w == i.s), ctx
        assert g.s_inv == cdiv(65536, g.s), ctx
        # two workgroups per CU only in the build that exists (kernels.hip: scan_variant): both tables as bytes
        assert g.wgs == 1 or (i.pair_byte and i.fc_byte), ctx
        if i.pin[0]:
            assert g.waves == i.pin[0], ctx
        if i.pin[1]:
            assert g.nch == i.pin[1], ctx
        # the 22-bit magic of the step: exact for every position of a tile where the plan says so, and where it does not, a
        # position that breaks it or a bound the planner asks for that fails
        magic = cdiv(1 << 22, g.s)
        assert g.s_magic22 == magic, ctx
        u = np.arange(positions, dtype=np.uint64)
        exact = bool(np.array_equal((u * np.uint64(magic)) >> np.uint64(22), u // np.uint64(g.s)))
        if g.div_exact:
            assert exact and not tips, ctx
        else:
            err = magic * g.s - (1 << 22)
            bounds = {"window scan": not tips, "magic < 2^24": magic < 1 << 24, "positions x magic < 2^32": positions * magic < 1 << 32,
                      "positions x error < 2^22": positions * err < 1 << 22}
            assert not exact or [name for name, holds in bounds.items() if not holds], ctx


def test_known_tilings_straight_from_the_core(host):
    for i, wpt in KNOWN:
        assert geometry(host, i, False).wpt == wpt, vars(i)
    g = geometry(host, KNOWN[0][0], False)
    assert (g.wgs, g.waves, g.nch) == (2, 10, 6)
    g = geometry(host, KNOWN[3][0], False)
    assert (g.wgs, g.waves, g.nch) == (1, 16, 7)
    assert host(["geom " + line(inputs(s=32768, w=32768, pin=(16, 8, 0, 0)), False)]) == ["geom nofit"]


# ------------------------------------------------------------------------------------------------------ tiles and ranges
def regions(n, tips, t):
    if n == 0:
        return []
    if not tips or n <= 2 * t:
        return [(0, n)]
    return [(0, t), (n - t, t)]


def plan_by_definition(i, tips, g, lens):
    """(tiles [(in_off, win_out, nrel, nwin, own_len, seg)], segs [(len, abs_pos, in_off, win_base, n_windows, first_tile, n_tiles)],
    input_bytes, n_windows)"""
    tb = g.wpt * g.s
    tiles, segs, off, wins = [], [], 0, 0
    for si, n in enumerate(lens):
        nw = 0 if tips else cdiv(n, i.s)
        first = len(tiles)
        for start, length in regions(n, tips, i.tl):
            for j, a in enumerate(range(0, length, tb)):
                rem = length - a
                tiles.append((off + start + a, 0 if tips else wins + j * g.wpt, min(rem, 1 << 30), 1 if tips else min(nw - j * g.wpt, g.wpt),
                              min(rem, tb), si))
        segs.append((n, 7 * si, off, 0 if tips else wins, nw, first, len(tiles) - first))
        off += a16(n)
        wins += nw
    return tiles, segs, off + IN_PAD, wins


def parse_tiles(text):
    head, rest = text.split(" :", 1)
    tiles, segs = rest.split(" |")
    input_bytes, n_windows, total, nt = map(int, head.split()[1:])
    tiles = [tuple(map(int, t.split(","))) for t in tiles.split()]
    assert len(tiles) == nt
    return tiles, [tuple(map(int, t.split(","))) for t in segs.split()], input_bytes, n_windows, total


def tile_cases(host):
    """[(inputs, tips, geometry, lens)]: segment lengths at the 16-byte, tile and tip edges"""
    out = []
    for i in (inputs(**HEADLINE), inputs(s=300, w=1000), inputs()):
        g = geometry(host, i, False)
        tb = g.wpt * g.s
        out.append((i, False, g, [0, 1, 15, 16, 17, tb - 1, tb, tb + 1, 3 * tb + 1]))
    for t in (100, 12000, 40000):
        i = inputs(tl=t)
        g = geometry(host, i, True)
        out.append((i, True, g, [0, 1, 15, 16, 17, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 5 * g.s + 3, g.s - 1, g.s, g.s + 1]))
    return out


def test_tiles_by_their_definitions(host):
    cases = tile_cases(host)
    lines = host(["tiles " + plan_line(i, tips, lens) for i, tips, _, lens in cases])
    for (i, tips, g, lens), text in zip(cases, lines):
        tiles, segs, input_bytes, n_windows, total = parse_tiles(text)
        want = plan_by_definition(i, tips, g, lens)
        assert (tiles, segs, input_bytes, n_windows) == want and total == sum(lens), (vars(i), tips, lens)
        for n, seg in zip(lens, segs):
            assert seg[4] == (0 if tips else cdiv(n, i.s)) and seg[2] % 16 == 0
    assert host(["tiles " + plan_line(inputs(), False, [])]) == ["tiles %d 0 0 0 : |" % IN_PAD]


def test_range_cover_of_every_range(host):
    for i, tips in ((inputs(**HEADLINE), False), (inputs(s=300, w=1000), False), (inputs(tl=12000), True)):
        g = geometry(host, i, tips)
        tb = g.wpt * g.s
        lens = [2 * tb + 17, 5, 0, 3 * tb, tb + 1, 33] if not tips else [2 * i.tl + 1 + 2 * tb, 5, 0, 3 * tb, 40001, tb + 1, 16]
        tiles, _, input_bytes, _, _ = parse_tiles(host(["tiles " + plan_line(i, tips, lens)])[0])
        nt = len(tiles)
        assert 8 <= nt <= 14
        head, rest = host(["cover " + plan_line(i, tips, lens)])[0].split(" :")
        got = [tuple(map(int, t.split(","))) for t in rest.split()]
        assert int(head.split()[1]) == nt and len(got) == (nt + 1) * (nt + 2) // 2
        at = 0
        for lo in range(nt + 1):
            for hi in range(lo, nt + 1):
                wb, we, ib, ie, bases = got[at]
                at += 1
                if lo == hi:
                    assert (wb, we, ib, ie, bases) == (0, 0, 0, 0, 0)
                    continue
                sel = tiles[lo:hi]
                assert bases == sum(t[4] for t in sel)
                assert (wb, we) == ((0, 0) if tips else (sel[0][1], max(t[1] + t[3] for t in sel)))
                assert ib % 16 == 0 and ib == sel[0][0] & ~15 and ie <= input_bytes
                # what the kernel loads for a tile: chunks of 2016 positions from the 16-byte boundary at or below its first base,
                # as many as hold its windows + halo (+ 16) or what is left of its region, + the 64 bytes the last lane reaches
                ends = []
                for in_off, _, nrel, nwin, _, _ in sel:
                    sh = in_off & 15
                    need = sh + min(nrel, (nwin + g.halo) * g.s + 16)
                    ends.append(in_off - sh + min(max(cdiv(need + 16, CHUNK), 1), g.nch) * CHUNK + 64)
                    assert ib <= in_off - sh
                assert ie == min(max(ends), input_bytes)


# ------------------------------------------------------------------------------------------------------------ the zone
def test_zone_words_are_isterminal_of_every_tile_position(host):
    """The kernel's compare (kernels.hip: finish_records) — a record at tile position u lies in the terminal zone iff
    u < zlo or u >= zhi, the two 16-bit halves of the tile's word — against isTerminal (rel <= t or rel >= N - t, the whole of a
    segment no longer than t) of the position, for every position a tile can hold; "the tile touches a zone" against "one of its
    owned positions is terminal".  300 000 and t = 70 000: lengths at which a threshold saturates at 0xFFFF."""
    saturated = set()
    for t in (1, 100, 12000, 70000):
        i = inputs(tl=t, **HEADLINE)
        g = geometry(host, i, False)
        positions = g.nch * CHUNK + 64
        lens = [n for n in (t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 2, 2 * t + 3 * g.wpt * g.s, 300000) if n > 0]
        tiles, segs, _, _, _ = parse_tiles(host(["tiles " + plan_line(i, False, lens)])[0])
        head, rest = host(["zone " + plan_line(i, False, lens)])[0].split(" :")
        per_tile, words = rest.split(" |")
        per_tile = [tuple(map(int, x.split(","))) for x in per_tile.split()]
        words = list(map(int, words.split()))
        assert len(per_tile) == len(tiles) and words == [x[2] for x in per_tile] + [ZONE_NONE]
        u = np.arange(positions, dtype=np.int64)
        zone_bases = 0
        for (in_off, _, _, _, own_len, seg), (lo, hi, word, touches) in zip(tiles, per_tile):
            n, rel0 = segs[seg][0], in_off - segs[seg][2]
            terminal = (rel0 + u <= t) | (rel0 + u >= (n - t if n > t else 0))
            zlo, zhi = word & 0xFFFF, word >> 16
            assert (zlo, zhi) == (min(lo, 0xFFFF), min(hi, 0xFFFF))
            saturated |= {("lo", lo > 0xFFFF), ("hi", hi > 0xFFFF)}
            assert np.array_equal((u < zlo) | (u >= zhi), terminal), (t, n, rel0)
            assert touches == int(terminal[:own_len].any()), (t, n, rel0)
            assert (word == ZONE_NONE) <= (not terminal.any())
            zone_bases += own_len if touches else 0
        assert int(head.split()[2]) == zone_bases
    assert {("lo", True), ("hi", True)} <= saturated


# --------------------------------------------------------------------------------------------- launch sizes and regrow
def visible_estimate(i, bases, zone):
    return int(bases * (max(i.ncanon, 1) / 4 ** min(i.k, 16)) * 1.5) + zone // 8


def zone_bases_of(i, tiles, segs):
    z = 0
    for in_off, _, _, _, own_len, seg in tiles:
        n, rel0 = segs[seg][0], in_off - segs[seg][2]
        if rel0 <= i.tl or rel0 + own_len > (n - i.tl if n > i.tl else 0):
            z += own_len
    return z


def test_launch_sizes(host):
    MiB64 = 64 << 20
    cases = []
    for i, tips in ((inputs(**HEADLINE), False), (inputs(), False), (inputs(tl=12000), True), (inputs(viscap=1001, **HEADLINE), False)):
        for lens in ([30011, 17, 400003], [MiB64], [MiB64 + 1], [3_000_000] * 40, []):
            for cap in (0, 1 << 20):
                for ncu in (0, 8, 256):
                    cases.append((i, tips, lens, cap, ncu))
    tile_lines = host(["tiles " + plan_line(i, tips, lens, cap, ncu) for i, tips, lens, cap, ncu in cases])
    plans = [parse_tiles(t) for t in tile_lines]
    ranges = [sorted({(0, len(p[0])), (len(p[0]) // 3, 2 * len(p[0]) // 3), (0, 0)}) for p in plans]
    launch = host(["launch %s %d %d" % (plan_line(i, tips, lens, cap, ncu), lo, hi) for (i, tips, lens, cap, ncu), rs in zip(cases, ranges) for lo, hi in rs])
    at = 0
    for (i, tips, lens, cap, ncu), (tiles, segs, input_bytes, n_windows, _), rs in zip(cases, plans, ranges):
        g = geometry(host, i, tips)
        for lo, hi in rs:
            head, tail = launch[at].split(" : ")
            at += 1
            grid, waves, region_cap, match_cap, dealt, vis_cap = map(int, head.split()[1:])
            win_lo, win_hi, in_lo, in_hi, bases = map(int, tail.split())
            ctx = (vars(i), tips, lens, cap, ncu, lo, hi)
            sel = tiles[lo:hi]
            assert bases == sum(t[4] for t in sel), ctx
            if (lo, hi) == (0, len(tiles)):
                assert (win_lo, win_hi, in_lo, in_hi) == (0, n_windows, 0, input_bytes), ctx
            assert grid == min(max(cdiv(len(sel), g.waves), 1), (ncu or 256) * g.wgs) and waves == grid * g.waves, ctx
            per_wave = [0] * waves
            for n, t in enumerate(sel):
                per_wave[n % waves] += t[4]
            worst = max([256] + per_wave)
            # dealt tiles exactly for ranges of at most 64 MiB without a capacity request; their regions hold the worst case
            assert dealt == int(bases <= MiB64 and not cap), ctx
            assert region_cap % 4 == 0 and 256 <= region_cap <= (worst + 3) & ~3 and match_cap == region_cap * waves, ctx
            want = worst if dealt else min(max(cdiv(cap or bases // 4 + 4096, waves), 256), worst)
            assert region_cap == (want + 3) & ~3, ctx
            assert vis_cap % 8 == 0, ctx
            if tips:
                assert vis_cap == 0, ctx
            elif i.viscap:
                assert vis_cap == (i.viscap + 7) & ~7, ctx
            else:
                vcap = 2 * cdiv(visible_estimate(i, bases, zone_bases_of(i, sel, segs)), waves) + 12 * cdiv(g.wpt * g.s, i.k) + 2048
                vcap = min(worst if dealt else vcap, max(worst, 256))
                assert vis_cap == (vcap + 7) & ~7, ctx


def test_regrown_capacities(host):
    worsts = [0, 1, 3, 255, 256, 257, 1000, 65535, 1 << 20, (1 << 31) - 1, 1 << 31]
    for w, text in zip(worsts, host(["regrow %d %d" % (w, w) for w in worsts])):
        region_cap, vis_cap = map(int, text.split()[1:])
        assert region_cap > w and vis_cap > w and region_cap % 4 == 0 and vis_cap % 8 == 0, w
        assert region_cap == (w + w // 8 + 64 + 3) & ~3 and vis_cap == (w + w // 8 + 64 + 7) & ~7, w


# ------------------------------------------------------------------------------------------------------------ shards
SHARD_FIELDS = ("own_lo own_hi ext_lo ext_hi seg_begin n_segs off_segs off_windows off_tilevis off_visible off_blocks bytes visible_capacity "
                "block_capacity window_bytes visible_bytes field_bits n_windows").split()


def parse_shard(text):
    head, rest = text.split(" :")
    cuts, parts = rest.split(" |")
    ctx_tiles, zone, margin, wire16 = map(int, head.split()[1:])
    return (ctx_tiles, zone, margin, wire16, list(map(int, cuts.split())),
            [SimpleNamespace(**dict(zip(SHARD_FIELDS, map(int, p.split(","))))) for p in parts.split()])


def test_shard_plan(host):
    from tests import shardpack
    cases = []
    for i, tips in ((inputs(tl=50000, **HEADLINE), False), (inputs(tl=3000, nuc=0, **HEADLINE), False), (inputs(tl=12000), True)):
        g = geometry(host, i, tips)
        tb = g.wpt * g.s
        margin_bases = (cdiv(i.tl + 1, tb) + max(2, cdiv(i.kdist + i.k + 1, tb) + 1)) * tb
        for lens in ([40 * margin_bases], [7001] * 60 + [25000, 24000], [2 * margin_bases - tb - 1, 10 * margin_bases, 17, 0, 3 * margin_bases]):
            cases.append((i, tips, g, lens))
    for i, tips, g, lens in cases:
        tiles, segs, _, _, _ = parse_tiles(host(["tiles " + plan_line(i, tips, lens)])[0])
        nt, tb = len(tiles), g.wpt * g.s
        ctx_want = 0 if tips else max(2, cdiv(i.kdist + i.k + 1, tb) + 1)
        zone_want = 0 if tips else cdiv(i.tl + 1, tb)
        for parts in (1, 2, 3, 5, 8):
            for scale in (1, 2):
                ctx_tiles, zone, margin, wire16, cuts, shards = parse_shard(host(["shard %s %d %d" % (plan_line(i, tips, lens), parts, scale)])[0])
                where = (vars(i), tips, lens, parts, scale)
                assert (ctx_tiles, zone, margin) == (ctx_want, zone_want, ctx_want + zone_want), where
                assert wire16 == int(g.nch * CHUNK + 64 <= 16384 and (tips or i.k * i.w <= 65535)), where
                assert len(cuts) == parts + 1 and cuts[0] == 0 and cuts[-1] == nt and cuts == sorted(cuts), where
                for c in cuts[1:-1]:
                    if 0 < c < nt:
                        f, n = segs[tiles[c][5]][5:7]
                        # a cut inside a segment keeps a margin from both its ends, unless the segment is shorter than two margins
                        assert c == f or tips or n < 2 * margin or (c - f >= margin and f + n - c >= margin), (where, c)
                for q, r in enumerate(shards):
                    assert (r.own_lo, r.own_hi) == (cuts[q], cuts[q + 1]), where
                    inside_lo = r.own_hi > r.own_lo and r.own_lo > 0 and segs[tiles[r.own_lo][5]][5] != r.own_lo
                    inside_hi = r.own_hi > r.own_lo and r.own_hi < nt and segs[tiles[r.own_hi][5]][5] != r.own_hi
                    assert r.ext_lo == r.own_lo - (ctx_tiles if inside_lo else 0) and r.ext_hi == r.own_hi + (ctx_tiles if inside_hi else 0), where
                    assert 0 <= r.ext_lo and r.ext_hi <= nt, where
                    own = tiles[r.own_lo:r.own_hi]
                    if own:
                        assert (r.seg_begin, r.n_segs) == (own[0][5], own[-1][5] - own[0][5] + 1), where
                        assert r.n_windows == (0 if tips else own[-1][1] + own[-1][3] - own[0][1]), where
                    else:
                        assert (r.n_segs, r.n_windows) == (0, 0), where
                    assert r.field_bits == i.w.bit_length(), where
                    assert r.window_bytes == (0 if tips else cdiv((7 if i.nuc else 3) * i.w.bit_length(), 8)), where
                    assert r.visible_bytes == (2 if wire16 else 4), where
                    own_bases = sum(t[4] for t in own)
                    vis = 0 if tips else visible_estimate(i, own_bases, zone_bases_of(i, own, segs)) + 65536
                    assert r.visible_capacity == (min(vis * scale, own_bases + 16) + 7) & ~7, where
                    assert r.block_capacity == min((16 * r.n_segs + 256) * scale, 1 << 24), where
                    # sections: 16-byte aligned, in order, none reaching into the next
                    offs = [r.off_segs, r.off_windows, r.off_tilevis, r.off_visible, r.off_blocks, r.bytes]
                    sizes = [r.n_segs * 64, r.n_windows * r.window_bytes, len(own) * 2, r.visible_capacity * r.visible_bytes, r.block_capacity * 64]
                    assert offs[0] == 128 and all(o % 16 == 0 for o in offs), where
                    assert all(a + n <= b < a + n + 16 for a, n, b in zip(offs, sizes, offs[1:])), where
                    info = SimpleNamespace(window_bytes=r.window_bytes, visible_capacity=r.visible_capacity, visible_bytes=r.visible_bytes,
                                           block_capacity=r.block_capacity, msg_bytes=r.bytes)
                    off = shardpack.sections(info, r.n_segs, len(own), r.n_windows)        # (asserts that its end is msg_bytes)
                    assert [off[n] for n in ("segs", "windows", "tilevis", "visible", "blocks")] == offs[:5], where


# ------------------------------------------------------------------------------------------------------ through the library
@pytest.mark.parametrize("cli, tips, npat", [("-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -x 1 -w 1000 -s 500 -r -g -e -m -i -t 3000", 0, 124),
                                             ("-c TTAGGG -r -t 12000", 1, 38)])
def test_the_library_plans_what_the_core_plans(host, monkeypatch, cli, tips, npat):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import parse_cli, user_input
    for name in ("TS_GEOMETRY", "TS_ACC_PER_WINDOW", "TS_STAGE_U32", "TS_VIS_CAP"):
        monkeypatch.delenv(name, raising=False)
    ui = user_input(parse_cli("x.fa " + cli), device=K.DEVICE_NONE)
    assert len(ui.patternInfo) == npat and ui.foldCase
    i = inputs(s=ui.step, w=ui.windowSize, tl=ui.terminalLimit, k=6, npat=npat, ncanon=2, nuc=int(ui.outGC or ui.outEntropy), kdist=ui.maxMatchDist)
    lens = [400003, 17, 0, 64513, 30011, 1_000_000]
    tiles, segs, input_bytes, n_windows, total = parse_tiles(host(["tiles " + plan_line(i, tips, lens)])[0])
    nt = len(tiles)
    tel = ta.Teloscope(ui)
    L = K.lib()
    b = L.ts_batch_create(tel._ctx.ptr, (C.c_uint64 * len(lens))(*lens), None, len(lens), tips, 0)
    assert b, tel._ctx.error()
    try:
        info = K.BatchInfo()
        assert L.ts_batch_get_info(b, C.byref(info)) == 0
        match_cap = int(host(["launch %s 0 %d" % (plan_line(i, tips, lens), nt)])[0].split()[4])
        assert (info.n_segments, info.total_bases, info.input_bytes, info.n_windows, info.n_tiles, info.match_capacity) == \
            (len(lens), total, input_bytes, n_windows, nt, match_cap)
        arr = (K.TileInfo * nt)()
        assert L.ts_batch_get_tiles(b, 0, nt, arr) == 0
        assert [(t.seg_index, t.seg_offset, t.first_window, t.n_windows, t.owned_bases) for t in arr] == \
            [(seg, in_off - segs[seg][2], win_out, 0 if tips else nwin, own) for in_off, win_out, _, nwin, own, seg in tiles]
        covers = [tuple(map(int, t.split(","))) for t in host(["cover " + plan_line(i, tips, lens)])[0].split(" :")[1].split()]
        r, at = K.RangeInfo(), 0
        for lo in range(nt + 1):
            for hi in range(lo, nt + 1):
                if (lo * 7 + hi) % 11 == 0 or (lo, hi) == (0, nt):
                    assert L.ts_batch_range_info(b, lo, hi, C.byref(r)) == 0
                    assert (r.tile_begin, r.tile_end, r.window_begin, r.window_end, r.input_begin, r.input_end, r.bases) == (lo, hi) + covers[at]
                at += 1
        s = K.ShardInfo()
        for parts, scale in ((1, 1), (3, 1), (3, 2), (8, 1)):
            ctx_tiles, _, _, _, _, shards = parse_shard(host(["shard %s %d %d" % (plan_line(i, tips, lens), parts, scale)])[0])
            for q, sh in enumerate(shards):
                assert L.ts_batch_shard_info(b, parts, q, scale, C.byref(s)) == 0
                assert (s.own_begin, s.own_end, s.ext_begin, s.ext_end, s.seg_begin, s.seg_end, s.msg_bytes, s.visible_capacity, s.block_capacity,
                        s.window_bytes, s.visible_bytes, s.context_tiles) == \
                    (sh.own_lo, sh.own_hi, sh.ext_lo, sh.ext_hi, sh.seg_begin, sh.seg_begin + sh.n_segs, sh.bytes, sh.visible_capacity,
                     sh.block_capacity, sh.window_bytes, sh.visible_bytes, ctx_tiles)
    finally:
        L.ts_batch_destroy(b)
        tel.close()


def test_drivers_and_host_program_share_one_source():
    """capi.cpp and shard.cpp call the core and keep no planner of their own; the terminal-zone rule, the visible-record estimate,
    the 14-bit predicate and the CU's LDS size each stand in one place; the core needs no HIP, no context and no environment."""
    text = {n: open(os.path.join(CSRC, n)).read() for n in ("capi.cpp", "shard.cpp", "capi_internal.hpp", "kernels.hip", "generic.hip",
                                                            "tiled_plan_core.h", "scan_lds_core.h", "ts_internal.h")}
    core, lds = text["tiled_plan_core.h"], text["scan_lds_core.h"]
    assert re.findall(r'#include "([^"]+)"', core) == ["general_plan_core.h", "scan_lds_core.h", "ts_internal.h"]
    assert re.findall(r'#include "([^"]+)"', lds) == ["ts_internal.h"]
    code = re.sub(r"//[^\n]*", "", core + lds)                                 # (comments may name the drivers' entry points)
    for banned in ("hip_runtime", "ts_ctx", "ts_batch", "getenv"):
        assert banned not in code, banned
    for use in ("tsplan::plan_batch(", "tsplan::plan_geometry(", "tsplan::set_range(", "tsplan::range_cover(", "tsplan::zone_words(",
                "tsplan::regrown_region_cap(", "tsplan::regrown_vis_cap(", "tsplan::wire16_ok(", "tsplan::shard_boundaries("):
        assert use in text["capi.cpp"], use
    for use in ("tsplan::shard_range(", "tsplan::shard_layout(", "tsplan::shard_geom("):
        assert use in text["shard.cpp"], use
    for name in ("capi.cpp", "shard.cpp"):
        for own in ("TS_CHUNK", "kOccupancy", "1u << 14", "160u * 1024u", "zone_bases +=", "d_canon", "0xFFFF)", "worst / 8", "align16u", "ts_k_lds_bytes"):
            assert own not in text[name], (name, own)
    assert "struct ts_batch : tsplan::TiledPlan" in text["capi_internal.hpp"]
    everything = re.sub(r"//[^\n]*", "", "".join(text.values()))               # code only: each rule's expression stands once
    assert everything.count("160u * 1024u") == 1 and "TS_CU_LDS_BYTES = 160u * 1024u" in lds
    assert everything.count("<= (1u << 14)") == 1 and everything.count("d_canon * 1.5") == 1 and everything.count("rel <= terminal_limit || rel >= term_end") == 1
    for name in ("kernels.hip", "generic.hip"):
        assert '#include "scan_lds_core.h"' in text[name] and "uint32_t align16(" not in text[name], name
    assert "slice_layout(const" not in text["kernels.hip"] and "ts_k_lds_bytes" not in everything
    host_src = open(os.path.join(ROOT, "tests", "cpp", "tiled_plan_host.cpp")).read()
    assert "teloscope_amd/csrc/tiled_plan_core.h" in host_src
