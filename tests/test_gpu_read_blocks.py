"""The read block report on the device: ts_batch_call_read_blocks + ts_batch_read_blocks (the terminal blocks of a tips-only
batch as ordered rows, blockcall.hip's walks in their counting and placing forms) on a tiled set and every general set, the
formatter by itself (ts_read_block_lines_format, read_blocks.hip) and the three chunk calls.  Every expectation is the CPU oracle's
(tests/readblocks.py) or, for handmade rows, plain Python; ts_batch_download_blocks is held against the same rows."""
import ctypes as C

import numpy as np
import pytest

from tests import harness as H
from tests import readblocks as B
from tests import readsets as R

pytestmark = pytest.mark.gpu

TILED = "-l 42"
FLAGS = [TILED] + R.SETS
IDS = ["tiled"] + R.SET_IDS


@pytest.fixture(scope="module")
def env():
    import torch

    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input

    class Env:
        pass
    e = Env()
    e.torch, e.ta, e.K, e.L, e.user_input = torch, ta, K, K.lib(), user_input
    return e


def read_filter(env, flags):
    return env.ta.ReadTelomereFilter(env.user_input(R.options(flags)))


def filter_ctx(rf):
    return rf._ctx.ptr


def shaped_reads(flags):
    """readsets.reads_for and, behind them: a telomere at the start only, at the end only, at both; two stretches at one side
    further apart than -d (500); telomere throughout; a block across position 4096; none.  More than 130 reads in all."""
    opts = R.options(flags)
    rng = np.random.default_rng(41)
    f, r = opts.canonical_fwd.encode(), opts.canonical_rev.encode()
    rnd = lambda n: R.random_bases(rng, n)                          # noqa: E731
    reads = list(R.reads_for(flags))
    for i in range(12):
        reads += [f * (20 + i) + rnd(900 + 37 * i), rnd(700 + 41 * i) + r * (20 + i), f * (15 + i) + rnd(1500 + i) + r * (25 + i),
                  f * 30 + rnd(650 + i) + f * 30 + rnd(800), (f * 800)[:3000 + i], rnd(4000 - 13 * i) + f * 60 + rnd(300), rnd(2000 + i)]
    assert len(reads) >= 130 and len(reads) % 64 != 0
    return reads


def create(env, ctx, lens, tips=1, capacity=0):
    arr = (C.c_uint64 * max(len(lens), 1))(*lens)
    b = env.L.ts_batch_create(ctx, arr, None, len(lens), tips, capacity)
    assert b, env.L.ts_last_error(ctx)
    return b


def call_rows(env, ctx, b):
    """ts_batch_call_read_blocks with the overflow protocol of ts_batch_read_pass -> (rows as a structured array, their bytes,
    whether the first status reported an overflow)"""
    L, K = env.L, env.K
    flag = C.c_int(7)
    assert L.ts_batch_call_read_blocks(b, None) == K.TS_OK, L.ts_last_error(ctx)
    assert L.ts_batch_read_pass_status(b, C.byref(flag)) == K.TS_OK and flag.value in (0, 1)
    first = flag.value
    if first:
        assert L.ts_batch_sync(b) == K.TS_OK, L.ts_last_error(ctx)
        assert L.ts_batch_call_read_blocks(b, None) == K.TS_OK, L.ts_last_error(ctx)
        assert L.ts_batch_read_pass_status(b, C.byref(flag)) == K.TS_OK and flag.value == 0
    n = C.c_uint64(0)
    rc = L.ts_batch_read_blocks(b, None, 0, C.byref(n))
    assert rc == (K.TS_ERR_INVALID_ARG if n.value else K.TS_OK)
    buf = np.full(n.value + 1, 0xA5, dtype=np.uint8).repeat(56).view(K.READ_BLOCK_DT)
    if n.value > 1:                                                 # a buffer one row short: nothing is copied
        assert L.ts_batch_read_blocks(b, C.c_void_p(buf.ctypes.data), n.value - 1, C.byref(n)) == K.TS_ERR_INVALID_ARG
        assert (buf.view(np.uint8) == 0xA5).all()
    assert L.ts_batch_read_blocks(b, C.c_void_p(buf.ctypes.data), n.value, C.byref(n)) == K.TS_OK, L.ts_last_error(ctx)
    assert (buf[n.value:].view(np.uint8) == 0xA5).all()
    rows = buf[:n.value].copy()
    return rows, rows.tobytes(), first


def as_tuples(rows):
    return [(int(r["segment"]), int(r["block"]["start"]), int(r["block"]["block_len"]), bytes(r["block"]["block_label"]),
             int(r["block"]["forward_count"]), int(r["block"]["reverse_count"]), int(r["block"]["canonical_count"]),
             int(r["block"]["non_canonical_count"])) for r in rows]


def scanned_batch(env, ctx, reads, tips=1, capacity=0):
    b = create(env, ctx, [len(s) for s in reads], tips, capacity)
    for i, s in enumerate(reads):
        assert env.L.ts_batch_upload(b, i, s) == env.K.TS_OK, env.L.ts_last_error(ctx)
    assert env.L.ts_batch_scan(b, None, None) == env.K.TS_OK, env.L.ts_last_error(ctx)
    return b


@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
def test_ordered_rows_equal_the_oracle_and_the_downloaded_blocks(env, flags):
    rf = read_filter(env, flags)
    ctx = filter_ctx(rf)
    assert bool(env.L.ts_uses_fast_path(ctx)) == (flags == TILED)
    reads = shaped_reads(flags)
    oracle = B.read_oracle(flags)
    exp = [(i,) + row for i, s in enumerate(reads) for row in B.block_rows(oracle, s)]
    per_read = np.bincount([e[0] for e in exp], minlength=len(reads))
    assert (per_read == 0).any() and (per_read == 1).any() and (per_read >= 2).any()
    assert any(e[1] < 4096 < e[1] + e[2] for e in exp)              # a block across a tile boundary
    b = scanned_batch(env, ctx, reads)
    try:
        rows, raw, _ = call_rows(env, ctx, b)
        rows2, raw2, _ = call_rows(env, ctx, b)                      # the call again: the same bytes
        out = (env.K.SegmentOut * len(reads))()
        assert env.L.ts_batch_download_blocks(b, out) == env.K.TS_OK, env.L.ts_last_error(ctx)
        down = []
        for i in range(len(reads)):
            tb = env.ta.SegmentData(out[i], True).terminalBlocks
            down += [(i, int(t["start"]), int(t["block_len"]), bytes(t["block_label"]), int(t["forward_count"]), int(t["reverse_count"]),
                      int(t["canonical_count"]), int(t["non_canonical_count"])) for t in tb]
        env.L.ts_free_segments(out, len(reads))
    finally:
        env.L.ts_batch_destroy(b)
    assert raw == raw2
    got = as_tuples(rows)
    assert got == exp
    assert got == down
    assert (rows["reserved"] == 0).all()


def test_overflowed_scan_goes_through_status_sync_and_again(env):
    flags = R.OVERFLOW_SET + " -l 30"
    rf = read_filter(env, flags)
    ctx = filter_ctx(rf)
    reads = R.overflow_reads()
    oracle = B.read_oracle(flags)
    exp = [(i,) + row for i, s in enumerate(reads) for row in B.block_rows(oracle, s)]
    b = scanned_batch(env, ctx, reads)
    try:
        rows, _, first = call_rows(env, ctx, b)
    finally:
        env.L.ts_batch_destroy(b)
    assert first == 1
    assert as_tuples(rows) == exp and exp


def test_tiled_scan_that_overflowed_its_record_regions(env):
    """A tiled batch with room for 4 096 records in all and dense reads: the guard raises the flag, no walk runs and the rows are
    refused until the status has been read clean; after ts_batch_sync the second call gives the oracle's rows."""
    rf = read_filter(env, TILED)
    ctx = filter_ctx(rf)
    opts = R.options(TILED)
    f, r = opts.canonical_fwd.encode(), opts.canonical_rev.encode()
    rng = np.random.default_rng(53)
    reads = [R.random_bases(rng, int(rng.integers(3000, 8000))) for _ in range(40)] + [f * 2500, r * 2500, f * 1000 + r * 1500] * 7
    oracle = B.read_oracle(TILED)
    exp = [(i,) + row for i, s in enumerate(reads) for row in B.block_rows(oracle, s)]
    b = scanned_batch(env, ctx, reads, capacity=4096)
    try:
        flag, n = C.c_int(7), C.c_uint64(99)
        assert env.L.ts_batch_call_read_blocks(b, None) == env.K.TS_OK, env.L.ts_last_error(ctx)
        assert env.L.ts_batch_read_blocks(b, None, 0, C.byref(n)) == env.K.TS_ERR_STATE         # the status has not been read
        assert env.L.ts_batch_read_pass_status(b, C.byref(flag)) == env.K.TS_OK and flag.value == 1
        assert env.L.ts_batch_read_blocks(b, None, 0, C.byref(n)) == env.K.TS_ERR_STATE         # ... and it was not clean
        assert env.L.ts_batch_sync(b) == env.K.TS_OK, env.L.ts_last_error(ctx)
        rows, _, first = call_rows(env, ctx, b)
    finally:
        env.L.ts_batch_destroy(b)
    assert first == 0
    assert as_tuples(rows) == exp and len(exp) >= 21


@pytest.mark.parametrize("flags", [TILED, R.SETS[0]], ids=["tiled", R.SET_IDS[0]])
def test_more_rows_than_the_room_the_call_began_with(env, flags):
    """Three reads of 800 stretches each, further apart than -d: well over a thousand blocks against a room of 2 n + 1024 rows — whoever reads
    the rows grows the room and the placing walks run again from the same places."""
    rf = read_filter(env, flags)
    ctx = filter_ctx(rf)
    opts = R.options(flags)
    f, r = opts.canonical_fwd.encode(), opts.canonical_rev.encode()
    rng = np.random.default_rng(59)
    reads = [b"".join(unit * 9 + R.random_bases(rng, 560) for _ in range(800)) for unit in (f, r, f)]
    oracle = B.read_oracle(flags)
    exp = [(i,) + row for i, s in enumerate(reads) for row in B.block_rows(oracle, s)]
    assert len(exp) > 2 * len(reads) + 1024
    b = scanned_batch(env, ctx, reads)
    try:
        rows, raw, _ = call_rows(env, ctx, b)
        rows2, raw2, _ = call_rows(env, ctx, b)
    finally:
        env.L.ts_batch_destroy(b)
    assert as_tuples(rows) == exp
    assert raw == raw2


def test_a_full_scan_batch_is_refused(env):
    opts = H.parse_cli("x -w 1000 -s 500")
    tel = env.ta.Teloscope(env.user_input(opts, device=0))
    ctx = tel._ctx.ptr
    b = scanned_batch(env, ctx, [b"CCCTAA" * 500], tips=0)
    try:
        assert env.L.ts_batch_call_read_blocks(b, None) == env.K.TS_ERR_INVALID_ARG
        n = C.c_uint64(0)
        assert env.L.ts_batch_read_blocks(b, None, 0, C.byref(n)) != env.K.TS_OK
    finally:
        env.L.ts_batch_destroy(b)


def format_rows(env, ctx, rows, names, read_lens, cap=None):
    """rows: [(segment, start, block_len, label, fwd, rev, can, noncan)] -> (rc, bytes needed, text)"""
    K, L = env.K, env.L
    arr = np.zeros(len(rows), dtype=K.READ_BLOCK_DT)
    for a, r in zip(arr, rows):
        a["segment"] = r[0]
        blk = a["block"]
        blk["start"], blk["block_len"], blk["block_label"] = r[1], r[2], r[3]
        blk["forward_count"], blk["reverse_count"], blk["canonical_count"], blk["non_canonical_count"] = r[4:8]
    blob = b"".join(names)
    off = np.cumsum([0] + [len(n) for n in names[:-1]]).astype(np.uint64)
    ln = np.array([len(n) for n in names], dtype=np.uint32)
    rl = np.array(read_lens, dtype=np.uint32)
    need = C.c_uint64(0)
    exp_len = sum(len(B.format_line(names[r[0]], r[1:], read_lens[r[0]])) for r in rows)
    cap = exp_len if cap is None else cap
    out = np.full(cap + 16, 0x5A, dtype=np.uint8)
    rc = L.ts_read_block_lines_format(ctx, C.c_void_p(arr.ctypes.data), len(rows), C.c_void_p(off.ctypes.data), C.c_void_p(ln.ctypes.data),
                                      C.c_void_p(rl.ctypes.data), blob, len(blob), C.c_void_p(out.ctypes.data), cap, C.byref(need))
    assert (out[cap:] == 0x5A).all()
    return rc, need.value, out[:cap].tobytes()


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 700])
def test_formatter_on_handmade_rows(env, n_rows):
    """700 rows under names of 300 bytes exceed a wave's staging area of 8 KiB: the bytewise path; the short names stay staged."""
    rf = read_filter(env, TILED)
    ctx = filter_ctx(rf)
    rng = np.random.default_rng(n_rows)
    n_segs = max(1, n_rows // 3)
    long_names = n_rows == 700
    names = [bytes(rng.integers(33, 127, size=(300 if long_names and s % 2 == 0 else s % 23), dtype=np.uint8)) for s in range(n_segs)]
    read_lens = [int(rng.integers(1, 1 << 32)) for _ in range(n_segs)]
    rows = []
    for i in range(n_rows):
        start = int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
        if i % 50 == 7:
            start = (1 << 64) - 1 - 77
        rows.append((min(i // 3, n_segs - 1), start, 77 if i % 50 == 7 else int(rng.integers(0, 1 << 32)) >> int(rng.integers(0, 32)), b"pq"[i & 1:][:1],
                     int(rng.integers(0, 1 << 32)), i, int(rng.integers(0, 1000)), 10 ** (i % 10)))
    exp = b"".join(B.format_line(names[r[0]], r[1:], read_lens[r[0]]) for r in rows)
    stats = (C.c_uint64 * 3)()
    assert env.L.ts_read_block_text_stats(ctx, stats) == env.K.TS_OK
    before = list(stats)
    rc, need, text = format_rows(env, ctx, rows, names, read_lens)
    assert rc == env.K.TS_OK, env.L.ts_last_error(ctx)
    assert need == len(exp) and text == exp
    assert env.L.ts_read_block_text_stats(ctx, stats) == env.K.TS_OK
    assert [int(a) - int(z) for a, z in zip(stats, before)] == [1, n_rows, len(exp)]
    rc, need, text = format_rows(env, ctx, rows, names, read_lens, cap=len(exp) - 1)     # too small: nothing is copied
    assert rc == env.K.TS_ERR_INVALID_ARG and need == len(exp) and set(text) <= {0x5A}


# ---- the chunk calls

def chunk_lines(env, ctx, kind, text, n_reads):
    """upload, walk, stage / decode, scan, call the blocks, format -> (the report's bytes, lines)"""
    K, L = env.K, env.L
    ch = L.ts_bam_chunk_create(ctx, 1 << 16, len(text) + 64)
    assert ch, L.ts_last_error(ctx)
    b = None
    try:
        assert L.ts_chunk_upload(ch, text, len(text), 0, None) == K.TS_OK, L.ts_last_error(ctx)
        u64 = lambda: C.c_uint64(0)                                 # noqa: E731
        n, nxt, err = u64(), u64(), C.c_int(0)
        if kind == "fastq":
            recs = (K.FastqRecord * n_reads)()
            e1, e2 = u64(), u64()
            assert L.ts_fastq_chunk_walk(ch, 1, recs, n_reads, C.byref(n), C.byref(nxt), C.byref(err), C.byref(e1), C.byref(e2)) == K.TS_OK
            lens = [r.seq_len - r.seq_cr for r in recs]
        elif kind == "sam":
            recs = (K.SamRecord * n_reads)()
            w = [u64() for _ in range(5)]
            assert L.ts_sam_chunk_walk(ch, 1, 1, recs, n_reads, C.byref(n), C.byref(w[0]), C.byref(w[1]), C.byref(w[2]), C.byref(nxt),
                                       C.byref(err), C.byref(w[3]), C.byref(w[4])) == K.TS_OK
            lens = [r.seq_len for r in recs]
        else:
            recs = (K.BamRecord * n_reads)()
            e1 = u64()
            assert L.ts_bam_chunk_walk(ch, 0, recs, n_reads, C.byref(n), C.byref(nxt), C.byref(err), C.byref(e1)) == K.TS_OK
            lens = [r.l_seq for r in recs]
        assert n.value == n_reads and err.value == 0 and nxt.value == len(text), (n.value, err.value, nxt.value)
        b = create(env, ctx, lens)
        stage = {"fastq": L.ts_fastq_chunk_stage, "sam": L.ts_sam_chunk_stage, "bam": L.ts_bam_chunk_decode}[kind]
        assert stage(ch, recs, n_reads, b, None) == K.TS_OK, L.ts_last_error(ctx)
        assert L.ts_batch_scan(b, None, None) == K.TS_OK, L.ts_last_error(ctx)
        call_rows(env, ctx, b)
        lines_call = {"fastq": L.ts_fastq_chunk_block_lines, "sam": L.ts_sam_chunk_block_lines, "bam": L.ts_bam_chunk_block_lines}[kind]
        need, n_lines = u64(), u64()
        rc = lines_call(ch, recs, n_reads, b, None, 0, C.byref(need), C.byref(n_lines), None)
        assert rc == K.TS_ERR_INVALID_ARG and need.value > 0
        small = np.full(need.value, 0x5A, dtype=np.uint8)
        assert lines_call(ch, recs, n_reads, b, C.c_void_p(small.ctypes.data), need.value - 1, C.byref(need), C.byref(n_lines), None) == K.TS_ERR_INVALID_ARG
        assert (small == 0x5A).all()
        out = np.full(need.value + 16, 0x5A, dtype=np.uint8)
        assert lines_call(ch, recs, n_reads, b, C.c_void_p(out.ctypes.data), need.value, C.byref(need), C.byref(n_lines), None) == K.TS_OK, L.ts_last_error(ctx)
        assert (out[need.value:] == 0x5A).all()
        return out[:need.value].tobytes(), n_lines.value
    finally:
        if b:
            L.ts_batch_destroy(b)
        L.ts_bam_chunk_destroy(ch)


@pytest.mark.parametrize("kind", ["fastq", "sam", "bam"])
@pytest.mark.parametrize("flags", [TILED, R.SETS[0]], ids=["tiled", R.SET_IDS[0]])
def test_chunk_block_lines_equal_the_reference_report(env, flags, kind):
    rf = read_filter(env, flags)
    ctx = filter_ctx(rf)
    reads = [r for r in shaped_reads(flags) if len(r) > 0]
    text, names = {"fastq": B.fastq_input, "sam": B.sam_input, "bam": B.bam_records}[kind](reads)
    exp, kept = B.ref_report(list(zip(names, reads)), B.read_oracle(flags))
    assert exp and len(kept) < len(reads)
    got, n_lines = chunk_lines(env, ctx, kind, text, len(reads))
    assert got == exp
    assert n_lines == exp.count(b"\n")
