"""ts_terminal_ends (Teloscope.terminalEnds): for every segment, the longest tips-only terminal block at its start side and at
its end side (walkSegment's distToStart <= distToEnd rule, src/input.cpp:849-853) — against the CPU oracle's terminal blocks
reduced per side, and at scale against ts_scan_segments_blocks' blocks reduced on the host."""
import numpy as np
import pytest

from tests import harness as H
from tests import seqgen

pytestmark = pytest.mark.gpu

FWD, REV = "CCCTAA", "TTAGGG"


def per_side(blocks, n, abs_pos):
    best = [0, 0]
    for b in blocks:
        rel, ln = int(b["start"]) - abs_pos, int(b["block_len"])
        side = 0 if rel <= n - (rel + ln) else 1
        best[side] = max(best[side], ln)
    return best


def segments(seed, t):
    """lengths from 1 base to several Mb; telomeric runs at the start, the end, both, neither or inside; lower case and N
    runs; runs long enough for the whole-wave walk (>= 128 records per list)"""
    rng = np.random.default_rng(seed)
    out = []
    lens = [1, 5, 11, 60, 150, 299, 301, 700, 999, 1001, 2 * t - 1, 2 * t + 1, 3 * t, 12000, 60000, 130000]
    for n in lens:
        for kind in range(6):
            s = bytearray(seqgen.random_dna(rng, n).tobytes())
            run = int(rng.integers(6, 4000))
            if kind in (1, 3):
                u = (FWD * (run // 6 + 1)).encode()[:min(run, n)]
                s[:len(u)] = u
            if kind in (2, 3):
                u = (REV * (run // 6 + 1)).encode()[:min(run, n)]
                s[n - len(u):] = u
            if kind == 4 and n > 500:
                a = int(rng.integers(0, n - 400))
                u = (REV * 60).encode()[:min(360, n - a)]
                s[a:a + len(u)] = u
            if kind == 5 and n > 100:
                u = (FWD * 40).encode().lower()[:n // 2]
                s[:len(u)] = u
                a = int(rng.integers(0, n - 20))
                s[a:a + 20] = b"N" * 20
            out.append(bytes(s))
    big = bytearray(seqgen.random_dna(rng, 3_000_000).tobytes())
    big[:20000] = (FWD * 4000).encode()[:20000]
    big[-9000:] = (REV * 1500).encode()
    big[1_500_000:1_503_000] = (REV * 500).encode()
    out.append(bytes(big))
    long_one = (FWD * 3000).encode() + seqgen.random_dna(rng, 5000).tobytes() + (REV * 3000).encode()   # wave walk when t is large
    out.append(long_one)
    return out


OPTIONS = [
    "-t 100 -l 60",
    "-t 300 -l 60",
    "-t 1000 -k 20 -d 100 -y 0.3",
    "-t 50000 -l 100",
    "-t 50000 -k 100 -l 60",
    "-t 1000 -x 1 -l 60 -c TTAGGG",
    "-t 300 -p CCCTAA,TTAGGG,CCCTAAA,TTTAGGG -l 60",     # mixed lengths: the general kernels' route
]


@pytest.mark.parametrize("rec32", [False, True], ids=["rec_auto", "rec32"])
@pytest.mark.parametrize("cli", OPTIONS)
def test_terminal_ends_match_oracle(cli, rec32, monkeypatch):
    import teloscope_amd as ta
    from teloscope_amd.cli import user_input
    from tests.backends import OracleBackend
    if rec32:
        monkeypatch.setenv("TS_REC32", "1")
    opts = H.parse_cli(cli + " dummy.fa")
    t = int(cli.split("-t ")[1].split()[0])
    seqs = segments(7 + t, t)
    abs_pos = [0 if i % 3 else 1_000_003 * i for i in range(len(seqs))]
    tel = ta.Teloscope(user_input(opts))
    got = tel.terminalEnds(seqs, abs_pos)
    orac = OracleBackend(opts)
    bad = []
    for i, s in enumerate(seqs):
        exp = per_side(orac.scan_segment(s.upper(), abs_pos[i], True)["terminal_blocks"], len(s), abs_pos[i])
        if list(got[i]) != exp:
            bad.append((i, len(s), list(got[i]), exp))
    assert got.shape == (len(seqs), 2) and got.dtype == np.uint32
    assert not bad, bad[:5]
    assert (got > 0).any()


def test_terminal_ends_rejects_full_scans():
    import ctypes as C
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    tel = ta.Teloscope(user_input(H.parse_cli("dummy.fa")))
    arr = (K.SegmentIn * 1)()
    arr[0].seq = b"CCCTAACCCTAA"
    arr[0].len = 12
    arr[0].tips_only = 0
    ends = (C.c_uint32 * 2)()
    assert K.lib().ts_terminal_ends(tel._ctx.ptr, arr, 1, ends) == K.TS_ERR_INVALID_ARG


@pytest.mark.parametrize("t", [1000, 50000])
def test_terminal_ends_equal_blocks_path_at_scale(t):
    """>= 200 000 segments of 50-2 000 bases (a pathless graph): ts_terminal_ends element by element equals the terminal
    blocks of ts_scan_segments_blocks on the same segments, reduced per side on the host"""
    import teloscope_amd as ta
    from teloscope_amd.cli import user_input
    rng = np.random.default_rng(11 + t)
    n = 200_000
    lens = rng.integers(50, 2001, n)
    pool = seqgen.random_dna(rng, int(lens.sum())).tobytes()
    cap = (FWD * 400).encode()
    tail = (REV * 400).encode()
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
    tel = ta.Teloscope(user_input(H.parse_cli("-t %d -l 60 dummy.fa" % t)))
    got = tel.terminalEnds(seqs)
    res = tel.scanSegmentsBlocksOnly([(s, 0) for s in seqs], tipsOnly=True)
    exp = np.array([per_side(r.terminalBlocks, len(s), 0) for r, s in zip(res, seqs)], dtype=np.uint32)
    assert (got > 0).sum() > n // 4
    assert np.array_equal(got, exp)
