#!/usr/bin/env python3
"""Dumps what the tiled scan's host plan decides, on a planning-only context (no GPU), as text on stdout: for a grid of parameter
sets and segment-length lists the TS_TIMING line of ts_batch_create (the geometry), every tile, ts_batch_range_info of several
ranges, ts_batch_shard_info for 1, 2, 3, 5 and 8 parts at scales 1 and 2, and ts_batch_get_info before and after a restriction.

Two builds of libteloscan.so plan alike exactly when their dumps are equal:

    TELOSCAN_LIB=/path/to/one/libteloscan.so   python profiles/tiled_plan_dump.py > a.txt
    TELOSCAN_LIB=/path/to/other/libteloscan.so python profiles/tiled_plan_dump.py > b.txt
    cmp a.txt b.txt

The last line counts the cases; profiles/tiled/plan_dump_parent_child.txt records one such comparison."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TS_TIMING"] = "1"
for name in ("TS_GEOMETRY", "TS_ACC_PER_WINDOW", "TS_STAGE_U32", "TS_VIS_CAP"):
    os.environ.pop(name, None)
os.dup2(1, 2)                                   # the library's stderr lines land in the dump, in order

import teloscope_amd as ta                      # noqa: E402
from teloscope_amd import _capi as K            # noqa: E402
from teloscope_amd.cli import parse_cli, user_input     # noqa: E402

HEADLINE = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -x 1 -w 1000 -s 500 -r -g -e -m -i"
# (cli, environment): the six of tests/test_capi_symbols.py::test_planner_tiling_choices first
SETS = [(HEADLINE, {}), ("-c TTAGGG -x 0 -w 1000 -s 500 -g -e -i", {}), ("-c TTAGGG -r -g -e -m -i", {}),
        ("-c CCCTAAA -w 2000 -s 1000 -r -g -e -m -i", {}), (HEADLINE, {"TS_GEOMETRY": "16,0"}),
        ("-c TTAGGG -r -g -e -m -i", {"TS_GEOMETRY": "10,6"}),
        ("-w 1000 -s 300 -g -e -m -i", {}), ("-w 1000 -s 300", {}), ("-w 32768 -s 32768 -g", {}), ("-w 32768 -s 16384 -g -e", {}),
        ("-w 6 -s 6 -g", {}), ("-w 12 -s 6 -g", {}), ("-w 300 -s 100 -g -e -m -i", {}), ("-t 3000", {}), ("-t 1", {}), ("-t 12000 -g", {})]
SETS += [("-c %s -w 1000 -s 500 -g -e" % "TTAGGGTT"[:k], {}) for k in range(3, 9)]
SETS += [("-c %s -x 1 -w 2000 -s 1000 -r" % "TTAGGGTT"[:k], {}) for k in range(3, 9)]
# the tilings tests/test_gpu_parity.py pins, over its parameter sets; the A/B flags
TILINGS = ["16,1", "16,3", "12,5", "10,6", "10,3", "8,2", "4,7", "2,4", "1,1", "1,8", "16,8,256", "12,6,0,2"]
for cli in ("-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -m -i", "-r -g -e -m -i",
            "-c CCCTAAA -w 2000 -s 1000 -r -g -e -m -i", "-w 300 -s 100 -g -e -m -i", "-t 3000"):
    SETS += [(cli, {"TS_GEOMETRY": t}) for t in TILINGS]
    SETS += [(cli, {"TS_ACC_PER_WINDOW": "1"}), (cli, {"TS_STAGE_U32": "1"}), (cli, {"TS_ACC_PER_WINDOW": "1", "TS_STAGE_U32": "1"})]

LENGTHS = [[3_000_000], [0, 1, 15, 16, 17, 30011, 400003, 64513, 2016, 4033, 129023, 1_000_000], [7001] * 60 + [25000, 24000, 23999],
           [], [150_000_000]]


def fields(s):
    return " ".join("%s=%s" % (n, getattr(s, n)) for n, _ in s._fields_ if not n.endswith("_ms"))


def dump_batch(L, ctx, lens, tips, cap):
    sys.stdout.flush()
    b = L.ts_batch_create(ctx, (C.c_uint64 * max(1, len(lens)))(*lens), (C.c_uint64 * max(1, len(lens)))(*[1000 * i for i in range(len(lens))]),
                          len(lens), tips, cap)
    if not b:
        print("refused:", L.ts_last_error(ctx).decode())
        return
    info = K.BatchInfo()
    assert L.ts_batch_get_info(b, C.byref(info)) == 0
    nt = int(info.n_tiles)
    print("info", fields(info), "wire16=%d" % L.ts_batch_wire16_ok(b))
    arr = (K.TileInfo * max(1, nt))()
    assert L.ts_batch_get_tiles(b, 0, nt, arr) == 0
    if nt <= 2000:
        for i in range(nt):
            print("tile", i, fields(arr[i]))
    else:                                        # a long plan: its ends, and a checksum of every field between them
        for i in list(range(8)) + list(range(nt - 8, nt)):
            print("tile", i, fields(arr[i]))
        acc = 0
        for i in range(nt):
            t = arr[i]
            acc = (acc * 1000003 + t.seg_index + 3 * t.seg_offset + 5 * t.first_window + 7 * t.n_windows + 11 * t.owned_bases) % (1 << 61)
        print("tiles", nt, "sum", acc)
    for i in range(len(lens)):
        print("segment_offset", i, L.ts_batch_segment_offset(b, i))
    r = K.RangeInfo()
    ranges = sorted({(0, nt), (0, min(1, nt)), (nt // 3, 2 * nt // 3), (max(nt - 1, 0), nt), (min(1, nt), nt), (nt // 2, nt // 2), (nt // 2, min(nt // 2 + 3, nt))})
    for lo, hi in ranges:
        assert L.ts_batch_range_info(b, lo, hi, C.byref(r)) == 0
        print("range", fields(r))
    s = K.ShardInfo()
    for parts in (1, 2, 3, 5, 8):
        for scale in (1, 2):
            for part in range(parts):
                assert L.ts_batch_shard_info(b, parts, part, scale, C.byref(s)) == 0
                print("shard scale=%d" % scale, fields(s))
        lo, hi = C.c_uint64(), C.c_uint64()
        assert L.ts_batch_partition(b, parts, parts - 1, C.byref(lo), C.byref(hi)) == 0
        print("partition", parts, lo.value, hi.value)
    for lo, hi in ranges[:4]:
        assert L.ts_batch_restrict(b, lo, hi) == 0
        assert L.ts_batch_get_info(b, C.byref(info)) == 0
        print("restricted", lo, hi, fields(info))
    L.ts_batch_destroy(b)


def main():
    L = K.lib()
    cases = 0
    for cli, env in SETS:
        os.environ.update(env)
        try:
            print("=== set %r env %r" % (cli, sorted(env.items())))
            try:
                tel = ta.Teloscope(user_input(parse_cli("x.fa " + cli), device=K.DEVICE_NONE))
            except Exception as exc:             # (a parameter set the front end or the library refuses is a line of the dump too)
                print("no context:", type(exc).__name__, exc)
                continue
            print("fast_path", int(tel.usesFastPath()))
            for lens in LENGTHS:
                for tips in (0, 1):
                    for cap in ((0, 1 << 20) if len(lens) == 1 else (0,)):
                        print("--- lens %s tips %d cap %d" % (lens if len(lens) < 20 else "%d lengths" % len(lens), tips, cap))
                        dump_batch(L, tel._ctx.ptr, lens, tips, cap)
                        cases += 1
            tel.close()
        finally:
            for name in env:
                del os.environ[name]
    print("cases", cases)


if __name__ == "__main__":
    main()
