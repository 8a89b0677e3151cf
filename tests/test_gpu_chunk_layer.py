"""The chunk layer under the device routes (teloscope_amd/csrc/chunk.cpp, chunk.hip, chunk_device.h), where the stage suites do
not look: the BAM gather's record copy at every size and alignment around its 16-byte stores, and one chunk object serving the
FASTQ, GFA and FASTA walks in turn, which pins the record of what the line index indexed.  References are the plain-Python ones
of tests/bamchunk.py, tests/fastqchunk.py, tests/fastachunk.py, tests/gfachunk.py and tests/filtercheck.py; equality is exact."""
import random
import struct
import types

import pytest

from tests import bamchunk as B
from tests import fastachunk as F
from tests import fastqchunk as FQ
from tests import filtercheck as FC
from tests import gfachunk as G
from tests import harness as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    rf = ta.ReadTelomereFilter(user_input(H.parse_cli("--fastq-subset -l 42"), device=0))
    yield types.SimpleNamespace(K=K, L=K.lib(), rf=rf, ctx=rf._ctx.ptr)
    rf.close()


# ------------------------------------------------------------------------------------------------ BAM gather placement
SIZES = list(range(36, 36 + 48))            # 4 + block_size: a 16-byte head, body and rest in every combination


def placement_records():
    """-> (plain, table).  Four rounds of the 48 sizes in one shuffled order; a round's bytes are a multiple of 4, and a record
    of 37 bytes in front of rounds 1, 2 and 3 moves every size's source offset through the four residues mod 4.  The records
    are handmade: a block_size field and bytes that no neighbour repeats."""
    order = random.Random(48).sample(SIZES, len(SIZES))
    sizes = []
    for r in range(4):
        sizes += ([37] if r else []) + order
    plain, table = bytearray(), []
    for i, s in enumerate(sizes):
        table.append((len(plain), s - 4, 36, 0))
        plain += struct.pack("<i", s - 4) + bytes((37 * i + 11 * k + 1) % 251 + 1 for k in range(s - 4))
    return bytes(plain), table


def test_bam_gather_places_every_size_at_every_alignment(env):
    K = env.K
    plain, table = placement_records()
    n = len(table)
    for s in SIZES:
        assert {off % 4 for off, bs, _, _ in table if 4 + bs == s} == {0, 1, 2, 3}, s
    assert sum(SIZES) % 4 == 0 and table[-1][0] + 4 + table[-1][1] == len(plain)
    # the last record ends on the last byte of the chunk's capacity: what the copy reads behind it is the buffer's slack
    chunk = FQ.Chunk(env.ctx, 1 << 16, len(plain))
    try:
        assert chunk.upload(plain, 0) == plain
        pats = {"all": [1] * n, "none": [0] * n, "alternating": [i & 1 for i in range(n)],
                "alternating from 0": [1 - (i & 1) for i in range(n)], "only the last": [0] * (n - 1) + [1]}
        d_pass = env.L.ts_bam_chunk_pass_buffer(chunk.ptr, n)
        assert d_pass
        seen = set()
        for name, p in pats.items():
            exp, kept = B.ref_gather(plain, table, p)
            to = 0
            for (off, bs, _, _), keep in zip(table, p):
                if keep:
                    seen.add((to % 16, 4 + bs))
                    to += 4 + bs
            B.to_device(d_pass, bytes(p))
            rc, out, nbytes, npassed = chunk.gather(table, d_pass, len(exp) + 64)
            assert (rc, nbytes, npassed) == (K.TS_OK, len(exp), kept), (name, rc, nbytes, npassed, env.L.ts_last_error(env.ctx))
            if out[:len(exp)] != exp:
                at = next(i for i, (a, b) in enumerate(zip(out, exp)) if a != b)
                raise AssertionError("%s: first difference at byte %d: %r, expected %r" % (name, at, out[at:at + 16], exp[at:at + 16]))
            assert out[len(exp):] == b"\xa5" * 64, "%s: the caller's buffer was written behind *bytes" % name
        assert len({a for a, _ in seen}) == 16 and {s for _, s in seen} == set(SIZES)
        assert chunk.read(0, len(plain)) == plain
    finally:
        chunk.close()


# ------------------------------------------------------------------------------------------------ one chunk, three routes
NOT_WALKED = "ts_gfa_chunk_check: ts_gfa_chunk_walk has not walked the chunk's bytes with this at_end"


def check_gfa(chunk, text, what):
    exp = G.ref_walk(text, True)
    rc, segs, lines, gathered, nxt, foreign, counts = chunk.gfa_walk(True, seg_cap=len(exp[0]) + 3, line_cap=len(exp[1]) + 3,
                                                                     text_cap=len(exp[2]) + 16)
    assert rc == chunk.K.TS_OK, chunk.L.ts_last_error(chunk.ctx)
    assert (segs, lines, gathered, nxt, foreign) == tuple(exp), what
    rc, n_lines, flagged, _ = chunk.gfa_check(True, cap=text.count(b"\n") + 2)
    assert rc == chunk.K.TS_OK, chunk.L.ts_last_error(chunk.ctx)
    assert (n_lines, flagged) == FC.ref_gfa_check(text, True), what


def test_one_chunk_serves_the_fastq_gfa_and_fasta_walks_in_turn(env):
    K = env.K
    fastq = FQ.reads_text(5, 6, lo=20, hi=50)
    gfa = FC.gfa_text([b"H\tVN:Z:1.0", b"S\ta\tACGTTAGGG\tLN:i:9", b"S\tb\t4\tACGT", b"L\ta\t+\tb\t-\t0M", b"X\tfoo", b"P\tp\ta+,b-\t*",
                       b"# a comment", b"S\tc\tTTAGGGTTAGGG"])
    # the FASTA text has the GFA text's length: the chunk's size alone does not say that its line index is another one
    fasta = b">r1 one\nACGTNNACGT\nAC\n>r2\nTTAGGG\r\n"
    fasta += b">r3\n" + b"A" * (len(gfa) - len(fasta) - 5) + b"\n"
    assert len(fasta) == len(gfa) and 300 > len(gfa) > 100 and len(fastq) > 100
    chunk = FC.Chunk(env.ctx, 1 << 16, 1 << 16)
    try:
        rc, n_lines, flagged, _ = chunk.gfa_check(True, cap=8)                 # (an empty chunk: nothing to check)
        assert (rc, n_lines, flagged) == (K.TS_OK, 0, [])
        chunk.upload(fastq, 0)
        assert chunk.fastq_walk(True) == FQ.ref_walk(fastq, True)
        rc, *_ = chunk.gfa_check(True, cap=8)                                  # a line index, but no GFA walk's
        assert rc == K.TS_ERR_INVALID_ARG and env.L.ts_last_error(env.ctx).decode() == NOT_WALKED
        chunk.reset()
        chunk.upload(gfa, 0)
        check_gfa(chunk, gfa, "the GFA walk behind the FASTQ walk")
        chunk.reset()
        chunk.upload(fasta, 0)
        rc, recs, nxt, names, _, _ = chunk.fasta_walk(True)
        assert rc == K.TS_OK and (recs, nxt, names) == F.ref_walk(fasta, True) and len(recs) == 3
        rc, n_lines, flagged, nf = chunk.gfa_check(True, cap=64)
        assert rc == K.TS_ERR_INVALID_ARG and env.L.ts_last_error(env.ctx).decode() == NOT_WALKED
        assert (n_lines, flagged, nf) == (0, [], 0)
        chunk.reset()
        chunk.upload(gfa, 0)
        check_gfa(chunk, gfa, "the GFA walk behind the FASTA walk")
        rc, *_ = chunk.gfa_check(False, cap=64)                                # not the at_end of the walk
        assert rc == K.TS_ERR_INVALID_ARG and env.L.ts_last_error(env.ctx).decode() == NOT_WALKED
    finally:
        chunk.close()
