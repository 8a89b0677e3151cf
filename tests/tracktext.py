"""Plain-Python reference for the text of the five window tracks (repeat density, canonical ratio, strand ratio, GC, entropy): what
BedWriter::format (include/teloscope_mi355x_io.hpp) writes per window, restated from the integer fields of a window record with
numpy float32 arithmetic and '%g' — no code shared with teloscope_amd/csrc/track_format_core.h, which the device formatter and its
host test program compile.  tests/test_track_format_core_cpu.py pins this file against harness.format_bed_files on the CPU
oracle's windows, and the core against it; the GPU tests compare the device's text with it.

A record is eight uint32 {A, C, G, T, canonical, non-canonical, forward, reverse covered}; a segment is
(first_window, n_windows, abs_pos, length, name bytes): window k of it covers [abs_pos + k * step, + min(w, length - k * step))."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from oracle import pyoracle
from tests.harness import _fmt_float

N_TRACKS = 5
DENSITY, CANON_RATIO, STRAND_RATIO, GC, ENTROPY = range(N_TRACKS)
SUFFIXES = ("_window_repeat_density.bedgraph", "_window_canonical_ratio.bedgraph", "_window_strand_ratio.bedgraph",
            "_window_gc.bedgraph", "_window_entropy.bedgraph")
f32 = np.float32

_entropy_memo = {}


def entropy(counts, size):
    """getShannonEntropy (include/teloscope.h:199-208) by the CPU oracle's own float32 code (log2f is libm's there as in the product)."""
    key = (tuple(int(c) for c in counts), int(size))
    v = _entropy_memo.get(key)
    if v is None:
        v = _entropy_memo[key] = f32(pyoracle.shannon_entropy(key[0], key[1]))
    return v


def column_values(rec, size, on):
    """The five column values of one window as float32 (None where the track is off): the expressions of BedWriter::format and
    getGCContent (include/teloscope.h:211-214: float division, double multiply by 100.0, narrowed)."""
    a, c, g, t, can, non, fwd, rev = (int(x) for x in rec)
    out = [None] * N_TRACKS
    with np.errstate(all="ignore"):
        if on[DENSITY]:
            tot = (fwd + rev) & 0xFFFFFFFF
            out[DENSITY] = f32(f32(tot) / f32(size))
            out[CANON_RATIO] = f32(f32(can) / f32((can + non) & 0xFFFFFFFF)) if tot > 0 else f32(-1.0)
            out[STRAND_RATIO] = f32(f32(fwd) / f32((fwd + rev) & 0xFFFFFFFF)) if tot > 0 else f32(-1.0)
        if on[GC]:
            out[GC] = f32(float(f32(f32((c + g) & 0xFFFFFFFF) / f32(size))) * 100.0)
        if on[ENTROPY]:
            out[ENTROPY] = entropy((a, c, g, t), size)
    return out


def track_switches(r, g, e):
    return [bool(r)] * 3 + [bool(g), bool(e)]


def window_lines(name, start, size, rec, on):
    """-> per track the window's line (bytes), or None"""
    pre = name + b"\t%d\t%d\t" % (start, start + size)
    return [None if v is None else pre + _fmt_float(v).encode() + b"\n" for v in column_values(rec, size, on)]


def format_tracks(records, segs, w, step, r, g, e):
    """records: (n, 8) uint32; segs: [(first_window, n_windows, abs_pos, length, name)] -> [bytes or None] * 5, None for a track
    that is off"""
    on = track_switches(r, g, e)
    parts = [[] for _ in range(N_TRACKS)]
    for first, n, abs_pos, length, name in segs:
        for k in range(n):
            size = min(w, length - k * step)
            assert size > 0
            for t, line in enumerate(window_lines(name, abs_pos + k * step, size, records[first + k], on)):
                if line is not None:
                    parts[t].append(line)
    return [b"".join(p) if on[t] else None for t, p in enumerate(parts)]


def format_windows(name, windows, r, g, e):
    """The same from expanded windows (ts_window / WindowData arrays: window_start, current_window_size, nucleotide_counts and the
    four covered counts — the integer fields only; the float fields are not read)."""
    on = track_switches(r, g, e)
    parts = [[] for _ in range(N_TRACKS)]
    for wd in windows:
        rec = [int(x) for x in wd["nucleotide_counts"]] + [int(wd["canonical_covered"]), int(wd["non_canonical_covered"]),
                                                           int(wd["fwd_covered"]), int(wd["rev_covered"])]
        for t, line in enumerate(window_lines(name, int(wd["window_start"]), int(wd["current_window_size"]), rec, on)):
            if line is not None:
                parts[t].append(line)
    return [b"".join(p) if on[t] else None for t, p in enumerate(parts)]


def n_windows(length, step):
    """windows of a fully scanned segment of `length` bases: one per step while a base is left (src/teloscope.cpp:537-658)"""
    return (length + step - 1) // step


def case_file(path, records, segs, w, step, r, g, e):
    """The input of `track_format_host tracks FILE` (tests/cpp/track_format_host.cpp)."""
    records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 8)
    names = b"".join(s[4] for s in segs)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<IIIIQQ", w, step, int(bool(r)) | 2 * int(bool(g)) | 4 * int(bool(e)), len(segs), len(records), len(names)))
        fh.write(records.tobytes())
        off = 0
        for first, n, abs_pos, length, name in segs:
            fh.write(struct.pack("<QQQQQII", first, n, abs_pos, length, off, len(name), 0))
            off += len(name)
        fh.write(names)


def parse_host_output(data):
    """stdout of `track_format_host tracks FILE` -> [bytes or None] * 5"""
    out, at = [], 0
    for t in range(N_TRACKS):
        end = data.index(b"\n", at)
        head = data[at:end].split()
        assert head[0] == b"#track" and int(head[1]) == t, data[at:end]
        at = end + 1
        if head[2] == b"-":
            out.append(None)
        else:
            out.append(data[at:at + int(head[2])])
            at += int(head[2])
    assert at == len(data)
    return out


# ------------------------------------------------------------------------------------------------ the library's stage, via ctypes
def device_format(tel, records, segs):
    """ts_window_tracks_format on the context of `tel` -> ([bytes or None] * 5, n_lines); raises TeloscanError on failure"""
    from teloscope_amd import _capi as K
    records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 8)
    names = b"".join(s[4] for s in segs)
    arr = (K.TrackSegment * max(1, len(segs)))()
    off = 0
    for i, (first, n, abs_pos, length, name) in enumerate(segs):
        arr[i].first_window, arr[i].n_windows, arr[i].abs_pos, arr[i].len = first, n, abs_pos, length
        arr[i].name_off, arr[i].name_len = off, len(name)
        off += len(name)
    text = K.TrackText()
    rc = K.lib().ts_window_tracks_format(tel._ctx.ptr, records.ctypes.data if len(records) else None, len(records), arr, len(segs),
                                         names, len(names), C.byref(text))
    if rc != K.TS_OK:
        raise K.TeloscanError(rc, tel._ctx.error())
    out = take_text(K, text)
    n_lines = int(text.n_lines)
    K.lib().ts_free_track_text(C.byref(text))
    assert all(not text.text[t] and text.len[t] == 0 for t in range(N_TRACKS))
    return out, n_lines


def take_text(K, text):
    """a ts_track_text's tracks as bytes; None for a track that came back NULL (then its length must be 0)"""
    out = []
    for t in range(N_TRACKS):
        if not text.text[t]:
            assert text.len[t] == 0
            out.append(None)
        else:
            out.append(C.string_at(text.text[t], int(text.len[t])))
    return out


def build_track_cli(out):
    """tests/cpp/track_text_cli.cpp against the built library -> the program's path"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "track_text_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)
