"""The host planning of the general kernels where no device is needed.  teloscope_amd/csrc/general_plan_core.h — the region rule,
the region tile planner and the whole-segment table entry that pipeline.cpp, general_batch.cpp and capi.cpp all call — run by a
program of its own under ASan + UBSan (tests/cpp/general_plan_host.cpp) against the rules restated here: the regions by the
sentence in tests/test_general_tile_cases_cpu.py ("[0, n) up to 2t bases, else [0, t) and [n - t, n)"), k_p0 and r_p0 by
division, avail by its definition.  And through the library: the tiles ts_batch_create plans for a tips-only batch on a
planning-only context are those regions, cut into the batch's tile size."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teloscope_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
HEADER = open(os.path.join(CSRC, "ts_internal.h")).read()
TILE = int(re.search(r"#define TS_GENERAL_TILE (\d+)", HEADER).group(1))
WIDE_HALO = int(re.search(r"#define TS_WIDE_HALO (\d+)", HEADER).group(1))
HAS_START, HAS_END = (int(re.search(r"#define TS_SEG_F_HAS_%s\s+(0x[0-9a-f]+)u" % n, HEADER).group(1), 16) for n in ("START", "END"))

LIMITS = (1, 31, 4095, 4096, 4097)


def edge_lengths(t):
    return (0, 1, t, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 2)


# ------------------------------------------------------------------------------------------------------- the rules, restated
def regions(n, tips, t):
    """[(start, length)] of a segment of n bases (terminal limits below 2^31: the product does not wrap)"""
    if n == 0:
        return []
    if not tips or n <= 2 * t:
        return [(0, n)]
    return [(0, t), (n - t, t)]


def tiles(in_off, start, length, seg, step, halo):
    """(in_off, seg_rel, k_p0, r_p0, n, avail, seg) per tile of a region"""
    out = []
    for a in range(0, length, TILE):
        n = min(TILE, length - a)
        k, r = divmod(start + a, step)
        out.append((in_off + a, start + a, k, r, n, min(length - a, n + halo), seg))
    return out


def entry(in_off, length, abs_pos, first_tile, n_tiles, seg):
    return (in_off, length, abs_pos, 0, length, first_tile, first_tile + n_tiles, first_tile, first_tile + n_tiles, HAS_START | HAS_END, seg)


# ------------------------------------------------------------------------------------------------ the core under sanitizers
@pytest.fixture(scope="module")
def host_plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("general_plan")
    exe = str(d / "general_plan_host")
    src = os.path.join(ROOT, "tests", "cpp", "general_plan_host.cpp")
    base = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    for extra in ([], ["-static-libasan"]):                        # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        if subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, timeout=60, env=ENV).returncode == 0:
            break
    return exe


def host_cases():
    """[(input line, expected output line)]"""
    cases = []

    def add(kind, args, want):
        cases.append(("%s %s" % (kind, " ".join(map(str, args))), want))

    def add_regions(n, tips, t):
        r = regions(n, tips, t)
        add("regions", (n, int(tips), t), "regions %d :%s" % (len(r), "".join(" %d,%d" % x for x in r)))

    def add_tiles(*args):
        t = tiles(*args)
        add("tiles", args, "tiles %d :%s" % (len(t), "".join(" " + ",".join(map(str, x)) for x in t)))

    for t in LIMITS + (2 ** 31 - 1,):
        for n in edge_lengths(t):
            add_regions(n, True, t)
            add_regions(n, False, t)
    # region lengths at the tile's edges and with a last tile shorter than the halo, under both halos
    for halo in (32, WIDE_HALO):
        for length in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, TILE + halo - 1, TILE + halo, TILE + halo + 1, 2 * TILE + 10):
            add_tiles(0, 0, length, 0, 500, halo)
            add_tiles(4112, 0, length, 3, 1, halo)
    # steps either side of the tile with starts that are no multiple of them: r_p0 carries zero, one and many times per tile
    for step in (1, 2, 997, TILE, TILE + 1, 2 * TILE - 1):
        for start in (5, 3 * step + 1, step - 1, 7 * step + step // 2, (1 << 33) + 12345):
            add_tiles(64, start, 5 * TILE + 17, 2, step, 32)
            add_tiles((1 << 40) + 16, start, 3 * TILE, 0xFFFFFFFF, step, WIDE_HALO)
    # the two tips of a segment in a batch's layout: the second one starts off a 16-byte boundary (and on one)
    for t, n in ((4097, 3 * 4097 + 2), (5000, 20011), (4096, 5 * 4096), (31, 100)):
        (a0, l0), (a1, l1) = regions(n, True, t)
        assert (a1 % 16 == 0) == (n in (5 * 4096,))
        for seg_off in (0, 48, 1 << 32):
            add_tiles(seg_off + a0, a0, l0, 1, 997, 32)
            add_tiles(seg_off + a1, a1, l1, 1, 997, 32)
    for args in ((0, 0, 0, 0, 0, 0), (48, 12345, 7, 3, 4, 9), (1 << 40, (1 << 36) + 5, 1 << 50, 0x7FFFFFF0, 15, 0xFFFFFFFE), (16, 1, 0, 5, 1, 0)):
        add("entry", args, "entry " + ",".join(map(str, entry(*args))))
    return cases


def test_core_equals_the_restated_rules_under_sanitizers(host_plan):
    cases = host_cases()
    r = subprocess.run([host_plan], input="".join(c[0] + "\n" for c in cases).encode(), capture_output=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    for line, (case, want) in zip(lines, cases):
        assert line == want, case


def test_drivers_and_host_program_share_one_source():
    for name in ("general_batch.cpp", "pipeline.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "general_plan_core.h"' in text, name
        for use in ("tsplan::scanned_regions(", "tsplan::append_region_tiles(", "tsplan::whole_segment_entry("):
            assert use in text, (name, use)
        for own in ("TsGeneralTile T", "k_p0", "r_p0", "T.avail", "TS_SEG_F_HAS_START"):       # no fill loop, no table entry of its own
            assert own not in text, (name, own)
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "tsplan::scanned_regions(" in capi and "tsplan::whole_segment_entry(" in capi and "TS_SEG_F_HAS_START | TS_SEG_F_HAS_END" not in capi
    host = open(os.path.join(ROOT, "tests", "cpp", "general_plan_host.cpp")).read()
    assert "teloscope_amd/csrc/general_plan_core.h" in host
    for use in ("tsplan::scanned_regions(", "tsplan::append_region_tiles(", "tsplan::whole_segment_entry("):
        assert use in host, use
    core = open(os.path.join(CSRC, "general_plan_core.h")).read()
    assert re.findall(r'#include "([^"]+)"', core) == ["ts_internal.h"] and "hip_runtime" not in core and "ts_ctx" not in core


# ------------------------------------------------------------------------------------------------------ through the library
def _batch_tiles(K, ctx, lens, tips=1):
    """[(segment, offset in it, owned bases)] of the plan ts_batch_create makes (ts_batch_get_tiles)"""
    L = K.lib()
    b = L.ts_batch_create(ctx, (C.c_uint64 * max(1, len(lens)))(*lens), None, len(lens), tips, 0)
    assert b, L.ts_last_error(ctx)
    try:
        info = K.BatchInfo()
        assert L.ts_batch_get_info(b, C.byref(info)) == 0
        arr = (K.TileInfo * max(1, info.n_tiles))()
        assert L.ts_batch_get_tiles(b, 0, info.n_tiles, arr) == 0
        return [(arr[i].seg_index, arr[i].seg_offset, arr[i].owned_bases) for i in range(info.n_tiles)]
    finally:
        L.ts_batch_destroy(b)


def _planning(limit):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import parse_cli, user_input
    return ta.Teloscope(user_input(parse_cli("x.fa -r -t %d" % limit), device=K.DEVICE_NONE))


@pytest.fixture(scope="module")
def tile_bases():
    """the tile size of a tips-only batch of the default pattern set: read off one region long enough to be cut"""
    from teloscope_amd import _capi as K
    tel = _planning(1 << 20)
    got = _batch_tiles(K, tel._ctx.ptr, [1 << 20])
    tel.close()
    size = got[0][2]
    assert len(got) > 2 and got == [(0, a, min(size, (1 << 20) - a)) for a in range(0, 1 << 20, size)]
    return size


@pytest.mark.parametrize("limit", LIMITS + (50000,))
def test_a_tips_batch_tiles_the_regions_of_the_rule(tile_bases, limit):
    from teloscope_amd import _capi as K
    tel = _planning(limit)
    try:
        assert tel.usesFastPath()
        lens = list(edge_lengths(limit)) + [2 * limit + 2 + 3 * tile_bases, 7]
        want = []
        for i, n in enumerate(lens):
            for start, length in regions(n, True, limit):
                want += [(i, a, min(tile_bases, start + length - a)) for a in range(start, start + length, tile_bases)]
        assert _batch_tiles(K, tel._ctx.ptr, lens) == want
        assert _batch_tiles(K, tel._ctx.ptr, []) == []
    finally:
        tel.close()
