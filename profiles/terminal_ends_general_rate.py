#!/usr/bin/env python3
"""ts_terminal_ends under -p TTAGGG,TTAGG (a mixed-length set: the general kernels) on the 200 000-segment pathless input of
tests/test_gpu_terminal_ends.py (segments of 50-2 000 bases, three in ten telomere-capped): two builds of libteloscan.so in
one process, a context each, the same segment array — the library given with --old (a build of the commit before the general
ENDS walk: the groups' blocks downloaded and reduced on the host) against the tree's.  One warm-up call of each, then the two
alternating three times, whole call; the answers compared every time; minimum and median of the three at the end.  Run on the
GPU box, under a time limit.
usage: profiles/terminal_ends_general_rate.py --old PATH [--out profiles/gfa/terminal_ends_general_rate.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from teloscope_amd import _capi as K                # noqa: E402
from teloscope_amd.cli import user_input           # noqa: E402
from tests import harness as H                      # noqa: E402
from tests import seqgen                            # noqa: E402

FWD, REV = "CCCTAA", "TTAGGG"


def segments(t=1000, n=200_000):
    rng = np.random.default_rng(11 + t)
    lens = rng.integers(50, 2001, n)
    pool = seqgen.random_dna(rng, int(lens.sum())).tobytes()
    cap, tail = (FWD * 400).encode(), (REV * 400).encode()
    seqs, at = [], 0
    for i, ln in enumerate(lens):
        s = pool[at:at + ln]
        at += ln
        r = i % 10
        if r == 1:
            s = cap[:ln // 2] + s[ln // 2:]
        elif r == 2:
            s = s[:ln - ln // 3] + tail[:ln // 3]
        elif r == 3:
            s = cap[:ln // 4] + s[ln // 4:ln - ln // 4] + tail[:ln // 4]
        seqs.append(s)
    return seqs


def bind(L):
    L.ts_create.restype = C.c_void_p
    L.ts_create.argtypes = [C.POINTER(K.Params), C.POINTER(K.Pattern), C.c_size_t]
    L.ts_destroy.argtypes = [C.c_void_p]
    L.ts_last_error.restype = C.c_char_p
    L.ts_last_error.argtypes = [C.c_void_p]
    L.ts_terminal_ends.argtypes = [C.c_void_p, C.POINTER(K.SegmentIn), C.c_size_t, C.POINTER(C.c_uint32)]
    L.ts_terminal_ends.restype = C.c_int
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gfa", "terminal_ends_general_rate.txt"))
    a = ap.parse_args()
    new = K.lib()
    libs = [("parent", bind(C.CDLL(os.path.abspath(a.old)))), ("this change", new)]
    ui = user_input(H.parse_cli("-t 1000 -l 60 -p TTAGGG,TTAGG dummy.fa"), device=0)
    params, (pats, npat) = ui._params(), ui._patterns()
    seqs = segments()
    n = len(seqs)
    arr = (K.SegmentIn * n)()
    for i, s in enumerate(seqs):
        arr[i].seq, arr[i].len, arr[i].abs_pos, arr[i].tips_only = s, len(s), 0, 1
    lines = ["ts_terminal_ends, -t 1000 -l 60 -p TTAGGG,TTAGG, %d segments, %d bases, whole call (host in, host out)" % (n, sum(map(len, seqs)))]
    ctxs = []
    for name, L in libs:
        ctx = L.ts_create(C.byref(params), pats, npat)
        if not ctx:
            raise SystemExit("%s: ts_create failed: %r" % (name, L.ts_last_error(None)))
        ctxs.append(ctx)
    walls = {name: [] for name, _ in libs}
    ref = None
    for rnd in range(4):                                 # round 0 is the warm-up
        for (name, L), ctx in zip(libs, ctxs):
            ends = np.zeros((n, 2), dtype=np.uint32)
            t0 = time.perf_counter()
            rc = L.ts_terminal_ends(ctx, arr, n, ends.ctypes.data_as(C.POINTER(C.c_uint32)))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != K.TS_OK:
                raise SystemExit("%s: ts_terminal_ends failed: %r" % (name, L.ts_last_error(ctx)))
            ref = ends if ref is None else ref
            if not np.array_equal(ends, ref):
                raise SystemExit("%s: the answer differs: the measurement ends here" % name)
            lines.append("%s %s: %.1f ms" % ("warm-up" if rnd == 0 else "run %d" % rnd, name, ms))
            if rnd:
                walls[name].append(ms)
    lines.append("segments with a terminal block: %d of %d; the two builds' answers are equal in every call" % (int((ref > 0).any(axis=1).sum()), n))
    for name, _ in libs:
        lines.append("%s: min %.1f ms, median %.1f ms of three" % (name, min(walls[name]), statistics.median(walls[name])))
    out = (C.c_uint64 * 4)()
    new.ts_terminal_ends_stats(ctxs[1], out)
    lines.append("this change, ts_terminal_ends_stats over its four calls: tiled %d, general %d, host %d segments, %d bytes device to host" % tuple(int(x) for x in out))
    for (name, L), ctx in zip(libs, ctxs):
        L.ts_destroy(ctx)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
