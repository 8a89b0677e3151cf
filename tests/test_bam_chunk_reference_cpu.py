"""The references of tests/bamchunk.py, pinned where no device is needed: ref_walk on hand-written streams whose answers are
literals, ref_decode on every byte value, the distribution of the walk fuzz's inputs, the carry plan's coverage of the four
moves, and the ts_bam_record mirror against the C compiler.  tests/test_gpu_bam_chunk.py compares the kernels with them."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import pytest

from tests import bamchunk as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_SEEDS = B.FUZZ_SEEDS


@pytest.mark.parametrize("case", B.verdict_cases(), ids=lambda c: c[0])
def test_ref_walk_hand_written_streams(case):
    _, stream, cap, expected = case
    assert B.ref_walk(stream, 0, cap) == expected


def test_verdict_cases_cover_every_verdict():
    cases = B.verdict_cases()
    assert {c[3][2] for c in cases} == {0, 1, 2, 3, 4}


def test_ref_walk_start_cap_and_tail():
    recs = [B.build_record(1 + i % 7, i % 3, i, seq=bytes((i + 1) // 2), aux=i % 5) for i in range(20)]
    stream = b"".join(recs)
    table, nxt, err, eoff = B.ref_walk(stream, 0, 100)
    assert (len(table), nxt, err, eoff) == (20, len(stream), 0, 0)
    assert [t[0] for t in table] == [sum(len(r) for r in recs[:i]) for i in range(20)]
    assert all(t[1] == len(r) - 4 and t[2] == 36 + 1 + i % 7 + 4 * (i % 3) and t[3] == i for i, (t, r) in enumerate(zip(table, recs)))
    assert B.ref_walk(stream, 0, 0) == ([], 0, 0, 0)
    assert B.ref_walk(stream, table[5][0], 3) == (table[5:8], table[8][0], 0, 0)
    for extra in (0, 1, 2, 3, 4, 35, 36):                            # a tail of `extra` bytes of one more record
        assert B.ref_walk(stream + recs[3][:extra], 0, 100) == (table, len(stream), 0, 0)
    assert B.ref_walk(stream, len(stream), 5) == ([], len(stream), 0, 0)


def test_ref_decode_every_byte_value():
    letters = "=ACMGRSVTWYHKDBN"
    for b in range(256):
        plain = bytes([b])
        assert B.ref_decode(plain, (0, 0, 0, 2)) == (letters[b >> 4] + letters[b & 15]).encode()
        assert B.ref_decode(plain, (0, 0, 0, 1)) == letters[b >> 4].encode()      # odd length: the low nibble is ignored
    plain = b"\xff" * 7 + bytes([0x12, 0x48, 0xf0]) + b"\xff"
    assert B.ref_decode(plain, (3, 0, 4, 5)) == b"ACGTN"
    assert B.ref_decode(plain, (3, 0, 4, 6)) == b"ACGTN="
    assert B.ref_decode(plain, (3, 0, 4, 0)) == b""


def test_ref_gather_and_member_packer():
    recs = [B.build_record(2, 0, i, seq=bytes((i + 1) // 2)) for i in range(6)]
    stream = b"".join(recs)
    table = B.ref_walk(stream, 0, 10)[0]
    assert B.ref_gather(stream, table, [0, 1, 0, 0, 7, 1]) == (recs[1] + recs[4] + recs[5], 3)
    assert B.ref_gather(stream, table, bytes(6)) == (b"", 0)
    plain = bytes(range(256)) * 600
    sizes = [0, 65536, 1, 0, 65535, 300]
    sizes.append(len(plain) - sum(sizes))
    for mode in ("stored", "zlib", "mixed"):
        comp, descs = B.pack_members(plain, sizes, mode)
        out = b""
        for (src, plen, isize, crc, dst), want in zip(descs, sizes):
            piece = zlib.decompress(comp[src:src + plen], -15)
            assert (len(piece), isize, dst, zlib.crc32(piece)) == (want, want, len(out), crc) and plen <= 65536
            out += piece
        assert out == plain


def test_fuzz_generator_distribution():
    """A condition on the inputs of the GPU fuzz: each verdict, and an incomplete last record, in at least an eighth of the
    streams (one mutation kind per seed % 6, so a sixth is what to expect)."""
    verdicts, incomplete = {v: 0 for v in range(5)}, 0
    for seed in range(FUZZ_SEEDS):
        stream, starts, kind = B.fuzz_stream(seed)
        assert kind == seed % 6 and starts[0] == 0
        _, nxt, err, _ = B.ref_walk(stream, 0, 1 << 20)
        verdicts[err] += 1
        incomplete += err == 0 and nxt < len(stream)
    assert all(n >= FUZZ_SEEDS // 8 for n in verdicts.values()), verdicts
    assert incomplete >= FUZZ_SEEDS // 8, incomplete
    assert [verdicts[v] for v in (1, 2, 3, 4)] == [FUZZ_SEEDS // 6] * 4


@pytest.mark.parametrize("first", [0, 8192, 8193, 40000])
def test_placement_streams_put_a_long_header_where_they_say(first):
    """Against a model of the walk's staging rule (B.staged_windows), not the builder's own arithmetic: when the walk
    reaches the placed record, the window it has staged ends exactly d bytes behind the record's start, and that window
    is a 1 KB one behind a block_size of 8 193 or 40 000 and a 16 KB one otherwise."""
    for d in range(301):
        stream, at = B.placement_stream(1000 * d + first, first, d)
        table, nxt, err, _ = B.ref_walk(stream, 0, 1 << 20)
        assert (nxt, err) == (len(stream), 0)
        assert [t for t in table if t[0] == at] and stream[at + B.AT_L_READ_NAME] == 255
        windows = B.staged_windows(stream)
        before = [w for w in windows if w[0] < at]
        pos, wlo, size = before[-1]                                  # the window staged when the walk arrives at the record
        assert wlo + size - at == d, (first, d, before)
        assert size == (1024 if first > 8192 else 16384)
        assert (1024 in [w[2] for w in windows]) == (first > 8192)
        if first:
            long_rec = [t for t in table if t[1] == first]
            assert len(long_rec) == 1 and pos == long_rec[0][0] + 4 + first     # forced by the record behind the long one
            assert len(before) == 2 and before[0] == (0, 0, 16384)
        else:
            assert before == [(0, 0, 16384)]
        # the record itself forces the next window exactly when its header region does not fit: a 16 KB one again
        forced = [w for w in windows if w[0] == at]
        assert bool(forced) == (d < 292) and all(w[2] == 16384 for w in forced)


def test_carry_plan_needs_every_move():
    stream, fills = B.carry_plan(7)
    assert 4 << 20 <= len(stream) <= 7 << 20 and sum(sum(s) for s, _ in fills) == len(stream)
    sizes = [s for f, _ in fills for s in f]
    assert 0 in sizes and 65536 in sizes and 1 <= min(s for s in sizes if s) and max(sizes) == 65536
    moves = B.simulate_carry(stream, fills)
    assert max(size for _, size in moves) <= 6 << 20
    kinds = [m for m, _ in moves]
    for kind in ("none", "in place", "direct", "through the temporary"):
        assert kinds.count(kind) >= 1, (kind, kinds)
    assert kinds[1:].count("none") >= 1                              # (not only the first fill of an empty chunk)


def test_bam_record_mirror_matches_header(tmp_path):
    from teloscope_amd import _capi as K
    src = tmp_path / "rec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "teloscan.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ts_bam_record), offsetof(ts_bam_record, off), '
                   'offsetof(ts_bam_record, block_size), offsetof(ts_bam_record, seq_at), offsetof(ts_bam_record, l_seq), '
                   'offsetof(ts_bam_record, reserved));'
                   'printf("%d %d %d %d %d\\n", TS_BAM_OK, TS_BAM_BAD_BLOCK_SIZE, TS_BAM_BAD_LENGTHS, TS_BAM_FIELDS_EXCEED, '
                   'TS_BAM_NAME_NOT_NUL);return 0;}')
    exe = tmp_path / "rec"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = K.BamRecord
    assert got == [C.sizeof(R), R.off.offset, R.block_size.offset, R.seq_at.offset, R.l_seq.offset, R.reserved.offset,
                   K.BAM_OK, K.BAM_BAD_BLOCK_SIZE, K.BAM_BAD_LENGTHS, K.BAM_FIELDS_EXCEED, K.BAM_NAME_NOT_NUL]
    assert got == [24, 0, 8, 12, 16, 20, 0, 1, 2, 3, 4]
    # the record builder lays the fields out where the walk reads them
    rec = B.build_record(9, 3, 11, seq=bytes(6), aux=5)
    assert struct.unpack_from("<i", rec, B.AT_BLOCK_SIZE)[0] == len(rec) - 4 == 32 + 9 + 12 + 6 + 11 + 5
    assert (rec[B.AT_L_READ_NAME], struct.unpack_from("<H", rec, B.AT_N_CIGAR_OP)[0], struct.unpack_from("<I", rec, B.AT_L_SEQ)[0]) == (9, 3, 11)
    assert rec[B.AT_NAME + 8] == 0 and 0 not in rec[B.AT_NAME:B.AT_NAME + 8]
