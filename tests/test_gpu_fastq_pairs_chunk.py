"""The two stages interleaved paired FASTQ adds to the device FASTQ route, one by one through ctypes against the plain references
of tests/fastqpairs.py (pinned without a device by tests/test_fastq_pairs_reference_cpu.py): ts_fastq_chunk_mates' lowest pair
that is not well formed, and ts_fastq_chunk_pair_pass' bytes, alone and as the d_pass of ts_fastq_chunk_gather.  Equality is exact
everywhere.  One context and one chunk serve the whole module; every case is a few hundred bytes to a few tens of KB of text.
tests/test_gpu_fastq_pairs_device.py checks the route as a whole."""
import types

import pytest

from tests import bamchunk as B
from tests import fastqchunk as F
from tests import fastqpairs as P
from tests import harness as H

pytestmark = pytest.mark.gpu
NONE = (1 << 64) - 1
GROUP = 64                                            # pairs a workgroup of the mates kernel takes
T = b"TTAGGG" * 6
N = b"ACGTCA" * 6


@pytest.fixture(scope="module")
def env():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("--fastq-subset -l 42")
    rf = ta.ReadTelomereFilter(user_input(opts, device=0))
    chunk = F.Chunk(rf._ctx.ptr, 64, 1 << 16)
    yield types.SimpleNamespace(K=K, L=K.lib(), rf=rf, ctx=rf._ctx.ptr, chunk=chunk)
    chunk.close()
    rf.close()


def held(env, text, at_end=True):
    """The text in the chunk and its record table, which must be the reference's."""
    env.chunk.reset()
    env.chunk.upload(text, 0)
    got, exp = env.chunk.fastq_walk(at_end, cap=max(16, len(text) // 8 + 16)), F.ref_walk(text, at_end)
    assert got == exp and got[2] == F.OK
    return got[0]


def check_every_pair(env, text, recs, what):
    """Every pair's verdict, by the lowest bad pair of the table from pair `start` on, `start` moved behind each one found."""
    assert len(recs) % 2 == 0
    start, bad = 0, []
    while True:
        rc, got = P.chunk_mates(env.chunk, recs[2 * start:])
        assert rc == env.K.TS_OK, env.L.ts_last_error(env.ctx)
        exp = P.ref_mismatch(text, recs[2 * start:])
        assert got == (NONE if exp is None else exp), "%s: from pair %d the lowest bad pair is %r, reference %r" % (what, start, got, exp)
        if exp is None:
            return bad
        bad.append(start + exp)
        start += exp + 1


RENDERINGS = [("lf", b"\n", b""), ("crlf", b"\r\n", b""), ("space", b"\n", b" 1:N:0 comment"), ("tab", b"\r\n", b"\tx y")]


@pytest.mark.parametrize("eol,end", [r[1:] for r in RENDERINGS], ids=[r[0] for r in RENDERINGS])
def test_mates_name_cases(env, eol, end):
    """Mate names of length 0 to 65, bare, with /1 + /2 and with the suffix on one mate; what is no suffix; names that differ in
    the first byte, the last byte or the length; ended by '\\n', "\\r\\n", a space and a tab.  The records lie behind one another,
    padded by the lengths in front: first and second mates begin on every residue modulo 16, the first at offset 0."""
    cases = P.name_cases()
    text = b"".join(F.record_text(a + end, T[:20 + i % 7], eol=eol) + F.record_text(b + end, N[:9 + i % 5], eol=eol) for i, (a, b, _, _) in enumerate(cases))
    recs = held(env, text)
    assert len(recs) == 2 * len(cases) and recs[0][0] == 0
    assert {r[0] % 16 for r in recs[0::2]} == set(range(16)) == {r[0] % 16 for r in recs[1::2]}
    assert {(r[0] + 1) % 4 for r in recs} == {0, 1, 2, 3}                       # the names begin at every place of a dword
    bad = check_every_pair(env, text, recs, "name cases")
    assert bad == [j for j, c in enumerate(cases) if not c[2]] and 20 < len(bad) < len(cases) - 40
    # ... and each pair alone in the table
    for j, (a, b, ok, what) in enumerate(cases):
        rc, got = P.chunk_mates(env.chunk, recs[2 * j:2 * j + 2])
        assert rc == env.K.TS_OK and got == (NONE if ok else 0), (what, a, b)


def test_mates_last_record_ends_on_the_chunks_last_byte(env):
    """No final newline: the last pair's second record ends where the chunk does, at every length of the chunk modulo 4, with
    records of one base (the name lies seven bytes in front of the chunk's end)."""
    for pad in range(4):
        for second, ok in ((b"ab/2", True), (b"ac/2", False), (b"ab", True)):
            text = F.record_text(b"p" * (1 + pad) + b"/1", T) + F.record_text(b"p" * (1 + pad), N) + F.record_text(b"ab/1", b"A") + b"@" + second + b"\nA\n+\nI"
            recs = held(env, text)
            assert len(recs) == 4 and recs[3][0] + recs[3][3] == len(text) == env.chunk.size()
            rc, got = P.chunk_mates(env.chunk, recs)
            assert rc == env.K.TS_OK and got == (NONE if ok else 1)
        text = F.record_text(b"x" * pad + b"/1", T) + F.record_text(b"x" * pad + b"/2", T)[:-1]
        recs = held(env, text)
        assert recs[1][0] + recs[1][3] == len(text) == env.chunk.size()
        assert P.chunk_mates(env.chunk, recs) == (env.K.TS_OK, NONE)


def pairs_text(n_pairs, bad=()):
    out = []
    for j in range(n_pairs):
        a, b = P.pair_names(j, P.STYLES[j % 3])
        if j in bad:
            b = b"q" + b[1:]
        out.append(F.record_text(a, T[:12 + j % 9]) + F.record_text(b, N[:7 + j % 11]))
    return b"".join(out)


@pytest.mark.parametrize("n_pairs", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1, 200])
def test_mates_pair_counts_and_lowest_mismatch(env, n_pairs):
    """Pair counts either side of one and two workgroups: no mismatch; one at pair 0; one at the last pair; two at once, of which
    the lowest wins — with 200 pairs they lie in different workgroups."""
    recs = held(env, pairs_text(n_pairs))
    assert len(recs) == 2 * n_pairs and P.chunk_mates(env.chunk, recs) == (env.K.TS_OK, NONE)
    two = (70, 135) if n_pairs == 200 else (n_pairs // 3, n_pairs - 1)
    assert n_pairs != 200 or two[0] // GROUP != two[1] // GROUP
    for bad in ((0,), (n_pairs - 1,), two, tuple(reversed(two))):
        text = pairs_text(n_pairs, bad)
        recs = held(env, text)
        assert P.ref_mismatch(text, recs) == min(bad)
        assert P.chunk_mates(env.chunk, recs) == (env.K.TS_OK, min(bad)), bad


def test_mates_arguments(env):
    text = pairs_text(3)
    recs = held(env, text)
    assert P.chunk_mates(env.chunk, recs[:5]) == (env.K.TS_ERR_INVALID_ARG, 7)
    assert P.chunk_mates(env.chunk, recs[:1]) == (env.K.TS_ERR_INVALID_ARG, 7)
    assert P.chunk_mates(env.chunk, []) == (env.K.TS_OK, NONE)
    # a record that does not lie inside the chunk is refused before anything is launched
    off, seq_at, seq_len, size, cr = recs[5]
    assert P.chunk_mates(env.chunk, recs[:5] + [(off, seq_at, seq_len, size + 2, cr)])[0] == env.K.TS_ERR_INVALID_ARG
    assert P.chunk_mates(env.chunk, recs[:5] + [(len(text), seq_at, seq_len, size, cr)])[0] == env.K.TS_ERR_INVALID_ARG
    assert P.chunk_mates(env.chunk, recs) == (env.K.TS_OK, NONE)


def pass_plan(n):
    """n records (n even): every combination of own pass bytes and of records that were not staged, cycling over the pairs ->
    (reads: b"" is a record without bases, read_of, the own pass bytes of the staged ones)"""
    kinds = [(1, 1), (1, 0), (0, 1), (0, 0), (None, 1), (None, 0), (1, None), (0, None), (None, None), (255, 0), (0, 2)]
    reads, read_of, own = [], [], []
    for j in range(n // 2):
        for v in kinds[j % len(kinds)]:
            if v is None:
                reads.append(b"")
                read_of.append(P.NOT_STAGED)
            else:
                reads.append(T if v else N)
                read_of.append(len(own))
                own.append(v)
    return reads, read_of, bytes(own)


@pytest.mark.parametrize("n", [2, 22, 126, 128, 130])
def test_pair_pass_and_gather(env, n):
    """All four own-pass combinations, a record that was not staged as first mate, as second and as both, pass bytes other than 1:
    the pair bytes are the reference's, d_pass is left as it was, and the gather over all n records with the pair bytes writes the
    reference's bytes."""
    reads, read_of, own = pass_plan(n)
    text = b"".join(F.record_text(b"p%d/%d" % (i // 2, 1 + i % 2), r) for i, r in enumerate(reads))
    recs = held(env, text)
    assert len(recs) == n and [r[2] > r[4] for r in recs] == [x != P.NOT_STAGED for x in read_of]
    at = (len(own) + 15) & ~15
    d_pass = env.L.ts_bam_chunk_pass_buffer(env.chunk.ptr, at + n)               # asked once: the two halves
    assert d_pass
    B.to_device(d_pass, own + b"\xee" * (at - len(own)) + b"\xee" * n)
    assert P.chunk_pair_pass(env.chunk, read_of, d_pass, d_pass + at) == env.K.TS_OK, env.L.ts_last_error(env.ctx)
    exp = P.ref_pair_pass(read_of, own)
    image = B.device_bytes(d_pass, at + n)
    assert image[at:] == exp and image[:at] == own + b"\xee" * (at - len(own))
    if n >= 22:
        assert {(exp[2 * j], read_of[2 * j] == P.NOT_STAGED, read_of[2 * j + 1] == P.NOT_STAGED) for j in range(n // 2)} == \
               {(1, False, False), (0, False, False), (1, True, False), (0, True, False), (1, False, True), (0, False, True), (0, True, True)}
    want, kept = F.ref_gather(text, recs, exp)
    rc, out, nbytes, npassed = env.chunk.fastq_gather(recs, d_pass + at, len(want) + 64)
    assert rc == env.K.TS_OK, env.L.ts_last_error(env.ctx)
    assert (nbytes, npassed) == (len(want), kept) and out[:nbytes] == want and out[nbytes:] == b"\xa5" * 64 and kept % 2 == 0


def test_pair_pass_arguments(env):
    reads, read_of, own = pass_plan(8)
    held(env, b"".join(F.record_text(b"p%d" % (i // 2), r) for i, r in enumerate(reads)))
    d_pass = env.L.ts_bam_chunk_pass_buffer(env.chunk.ptr, 64)
    B.to_device(d_pass, own + b"\xee" * (64 - len(own)))
    bad = env.K.TS_ERR_INVALID_ARG
    assert P.chunk_pair_pass(env.chunk, read_of[:7], d_pass, d_pass + 16) == bad
    assert P.chunk_pair_pass(env.chunk, read_of, d_pass, d_pass) == bad                     # must not alias
    assert P.chunk_pair_pass(env.chunk, [0, 8, 1, 2, 3, 4, 5, 6], d_pass, d_pass + 16) == bad   # behind the judged reads
    assert P.chunk_pair_pass(env.chunk, [], d_pass, d_pass + 16) == env.K.TS_OK
    assert B.device_bytes(d_pass, 64) == own + b"\xee" * (64 - len(own))                     # nothing was written
