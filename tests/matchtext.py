"""Plain-Python reference for the text of the two match files (_canonical_matches.bed, _noncanonical_matches.bed): what
BedWriter::format (include/teloscope_mi355x_io.hpp) writes per MatchInfo, restated from match records (position, size, flags), a
segment table and the bases — no code shared with teloscope_amd/csrc/match_format_core.h, which the device formatter and its host
test program compile.  tests/test_match_format_core_cpu.py pins this file against harness.format_bed_files on the CPU oracle's
matches, and the core against it; the GPU tests compare the device's text with it.

A record is (position, size, flags) with flags & 2 = canonical (TS_MATCH_CANONICAL; the terminal bit is NOT read); a segment is
(first_record, n_records, abs_pos, length, base_off, name bytes, tips_only): its bases are bases[base_off : base_off + length].
A full-scan record gives a canonical line if it is canonical, a non-canonical line if it is not and its position relative to its
segment is terminal (rel <= limit or rel >= max(length - limit, 0), src/teloscope.cpp:451-459), no line otherwise."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

N_FILES = 2
CANONICAL, NONCANONICAL = range(N_FILES)
SUFFIXES = ("_canonical_matches.bed", "_noncanonical_matches.bed")
MATCH_CANONICAL = 2


def is_terminal(rel, length, limit):
    return rel <= limit or rel >= (length - limit if length > limit else 0)


def format_matches(records, segs, bases, limit):
    """records: sequence of (position, size, flags); segs as above -> ([bytes, bytes], [lines, lines])"""
    parts, lines = [[], []], [0, 0]
    for first, n, abs_pos, length, base_off, name, tips_only in segs:
        if tips_only:
            continue
        for j in range(first, first + n):
            pos, size, flags = (int(x) for x in records[j])
            rel = pos - abs_pos
            assert 0 <= rel and rel + size <= length and 1 <= size <= 63
            if flags & MATCH_CANONICAL:
                f = CANONICAL
            elif is_terminal(rel, length, limit):
                f = NONCANONICAL
            else:
                continue
            seq = bases[base_off + rel:base_off + rel + size].upper()
            parts[f].append(name + b"\t%d\t%d\t" % (pos, pos + size) + seq + b"\n")
            lines[f] += 1
    return [b"".join(p) for p in parts], lines


def format_scanned(name, matches, abs_pos, seq, limit):
    """The same from one full-scan segment's ts_match array (numpy MATCH_DT: position, match_size, flags) and its bases."""
    recs = [(int(m["position"]), int(m["match_size"]), int(m["flags"])) for m in matches]
    return format_matches(recs, [(0, len(recs), abs_pos, len(seq), 0, name, False)], seq, limit)


# ------------------------------------------------------------------------------------------------ the generated case
NAME_LENS = (1, 15, 16, 17, 70, 300)
SIZES = (1, 3, 6, 8, 32, 63)
CASE_LIMIT = 300


def _bases(rng, n):
    """mixed-case ACGT with a few other letters"""
    return bytes(rng.choice(np.frombuffer(b"ACGTacgtACGTacgtNn", dtype=np.uint8), size=n).tobytes())


def generated_case(seed=20261019, limit=CASE_LIMIT):
    """-> (records, segs, bases): every digit count of position and end from 1 to 20 with the pairs where the end has one digit
    more; sizes 1, 3, 6, 8, 32, 63; names of 1, 15, 16, 17, 70, 300 bytes; lower- and mixed-case bases; records at limit,
    limit + 1, term_end - 1, term_end; a segment no longer than the limit and one between limit and 2 limit (all terminal);
    records skipped between segments; a tips-only segment; an empty segment.  Every record in a canonical and a non-canonical copy."""
    rng = np.random.default_rng(seed)
    records, segs, bases = [], [], []
    nseg = [0]

    def add_segment(abs_pos, length, recs, tips_only=False, skip=0):
        base_off = sum(len(b) for b in bases)
        bases.append(_bases(rng, length))
        ln = NAME_LENS[nseg[0] % len(NAME_LENS)]
        name = (b"s%d_" % nseg[0] + b"n" * 300)[:ln]
        nseg[0] += 1
        for _ in range(skip):                                        # records that belong to no segment
            records.append((abs_pos, 6, MATCH_CANONICAL))
        first = len(records)
        for rel, size in recs:
            assert rel + size <= length
            records.append((abs_pos + rel, size, MATCH_CANONICAL | int(rng.integers(0, 2))))
            records.append((abs_pos + rel, size, int(rng.integers(0, 2)) | 4 * int(rng.integers(0, 2))))
        segs.append((first, len(records) - first, abs_pos, length, base_off, name, tips_only))

    # positions around every power of ten: 10^d - 3 .. + 6 crosses a digit count, 10^d itself starts one
    add_segment(0, 200, [(0, 1), (0, 6), (3, 6), (4, 6), (9, 1), (9, 3), (9, 6), (10, 8), (94, 6), (97, 6), (99, 1), (100, 32), (137, 63)])
    for d in range(3, 20):
        p = 10 ** d
        add_segment(p - 100, 200, [(94, 6), (97, 6), (99, 1), (100, SIZES[d % 6]), (101, 63)])
    top = (1 << 64) - 1
    add_segment(top - 200, 200, [(0, 6), (100, 63), (137, 63), (194, 6)])       # 20-digit positions and ends
    # the terminal rule: interior records between limit + 1 and term_end - 1 give no non-canonical line
    n = 1000
    add_segment(5_000, n, [(0, 6), (limit - 1, 6), (limit, 6), (limit + 1, 6), (limit + 2, 3), (500, 8), (n - limit - 1, 6), (n - limit, 6),
                           (n - limit + 1, 32), (n - 63, 63), (n - 1, 1)], skip=3)
    add_segment(7_000, limit - 50, [(0, 6), (100, 6), (limit - 56, 6)])          # len <= limit: everything is terminal
    add_segment(7_500, limit, [(0, 6), (limit - 6, 6)])
    add_segment(8_000, limit + 150, [(0, 6), (149, 6), (150, 6), (151, 6), (limit, 6), (limit + 1, 6), (limit + 144, 6)], skip=1)
    add_segment(9_000, 400, [(0, 6), (200, 6)], tips_only=True)                  # no lines
    add_segment(9_500, 10, [])
    return records, segs, b"".join(bases)


def counted_case(counts, seed=3, limit=CASE_LIMIT, long_name=False):
    """Segments of the given record counts (0, 1, 63, 64, 65, 200, ...): every record of 6 bases, three in four canonical."""
    rng = np.random.default_rng(seed)
    records, segs, bases, off = [], [], [], 0
    for i, cnt in enumerate(counts):
        length = 6 * cnt + 700
        name = b"a_name_beyond_the_staging_area_" + b"x" * 200 if long_name and i % 2 else b"seq%d" % i
        first = len(records)
        for j in range(cnt):
            records.append((10_000 * i + 350 + 6 * j if j % 3 else 10_000 * i + j, 6, 0 if j % 4 == 3 else MATCH_CANONICAL))
        segs.append((first, cnt, 10_000 * i, length, off, name, False))
        bases.append(_bases(rng, length))
        off += length
    return records, segs, b"".join(bases)


def records_array(records):
    """-> numpy array in ts_match's layout"""
    dt = np.dtype([("position", "<u8"), ("match_size", "<u2"), ("flags", "u1"), ("reserved", "u1", (5,))])
    arr = np.zeros(len(records), dtype=dt)
    for i, (p, s, f) in enumerate(records):
        arr[i]["position"], arr[i]["match_size"], arr[i]["flags"] = p, s, f
    return arr


def case_file(path, records, segs, bases, limit):
    """The input of `match_format_host lines FILE` (tests/cpp/match_format_host.cpp)."""
    names = b"".join(s[5] for s in segs)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<IIQQQ", limit, len(segs), len(records), len(names), len(bases)))
        fh.write(records_array(records).tobytes())
        off = 0
        for first, n, abs_pos, length, base_off, name, tips in segs:
            fh.write(struct.pack("<QQQQQQII", first, n, abs_pos, length, base_off, off, len(name), int(tips)))
            off += len(name)
        fh.write(names)
        fh.write(bases)


def parse_host_output(data):
    """stdout of `match_format_host lines FILE` -> ([bytes, bytes], [lines, lines])"""
    out, lines, at = [], [], 0
    for f in range(N_FILES):
        end = data.index(b"\n", at)
        head = data[at:end].split()
        assert head[0] == b"#file" and int(head[1]) == f, data[at:end]
        at = end + 1
        out.append(data[at:at + int(head[2])])
        lines.append(int(head[3]))
        at += int(head[2])
    assert at == len(data)
    return out, lines


# ------------------------------------------------------------------------------------------------ the library's stage, via ctypes
def take_text(K, text):
    """a ts_match_text's files as bytes; None for a file that came back NULL (then its length must be 0)"""
    out = []
    for f in range(N_FILES):
        if not text.text[f]:
            assert text.len[f] == 0
            out.append(None)
        else:
            out.append(C.string_at(text.text[f], int(text.len[f])))
    return out


def device_format(tel, records, segs, bases, text=None):
    """ts_match_lines_format on the context of `tel` -> ([bytes or None] * 2, [lines] * 2); raises TeloscanError on failure.
    text: a ts_match_text to reuse (left holding the result), else one of the call's own, freed."""
    from teloscope_amd import _capi as K
    names = b"".join(s[5] for s in segs)
    arr = (K.MatchLineSegment * max(1, len(segs)))()
    off = 0
    for i, (first, n, abs_pos, length, base_off, name, tips) in enumerate(segs):
        arr[i].first_record, arr[i].n_records, arr[i].abs_pos, arr[i].len, arr[i].base_off = first, n, abs_pos, length, base_off
        arr[i].name_off, arr[i].name_len, arr[i].tips_only = off, len(name), int(tips)
        off += len(name)
    recs = records_array(records)
    own = text is None
    if own:
        text = K.MatchText()
    rc = K.lib().ts_match_lines_format(tel._ctx.ptr, recs.ctypes.data if len(recs) else None, len(recs), arr, len(segs), names, len(names),
                                       bases, len(bases), C.byref(text))
    if rc != K.TS_OK:
        assert all(not text.text[f] and text.len[f] == 0 and text.capacity[f] == 0 for f in range(N_FILES))    # empty after a failure
        raise K.TeloscanError(rc, tel._ctx.error())
    out, lines = take_text(K, text), [int(text.n_lines[f]) for f in range(N_FILES)]
    if own:
        K.lib().ts_free_match_text(C.byref(text))
        assert all(not text.text[f] and text.len[f] == 0 for f in range(N_FILES))
    return out, lines


def build_match_cli(out):
    """tests/cpp/match_text_cli.cpp against the built library -> the program's path"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "match_text_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)
