"""ts_scan_segments_tracks against ts_scan_segments_blocks on the same segments and context: blocks and counts are equal, no
window records come back, and the text of every track equals tests/tracktext.py applied to the integer fields of the windows
ts_scan_segments_blocks expands on the host — for host and device-resident segments, tips-only segments mixed in (no lines), the
tiled kernel, the general kernels (a mixed-length pattern set, and the tiled set under TS_FORCE_GENERAL=1) and a call that spans
two pipeline groups."""
import ctypes as C

import numpy as np
import pytest

from tests import seqgen
from tests import tracktext as T
from tests.test_gpu_input_device import make, segments_in

pytestmark = pytest.mark.gpu

TILED = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -i"
LIST_FORM = "-p TTAGGG,TTAGG -w 1000 -s 500 -r -g -e -i"


def planted(rng, n):
    """n random bases with TTAGGG / CCCTAA arrays and N-runs planted where they fit"""
    s = seqgen.random_dna(rng, n).copy()
    if n >= 400:
        k = min(n // 5, 1200) // 6 * 6
        s[:k] = seqgen.mutate(rng, seqgen.repeat_array("CCCTAA", k // 6), 0.02)
        s[n - k:] = seqgen.mutate(rng, seqgen.repeat_array("TTAGGG", k // 6), 0.02)
    if n >= 3000:
        a = int(rng.integers(n // 3, n // 2))
        s[a:a + 300] = seqgen.repeat_array("TTAGGG", 50)
        s[a + 700:a + 700 + 1234] = ord("N")
    elif n >= 20:
        s[n // 2:n // 2 + 3] = ord("N")
    return s.tobytes()


def blocks_call(tel, specs):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    keep, n = [], len(specs)
    arr = segments_in(K, specs, keep)
    out, cnt = (K.SegmentOut * max(1, n))(), (K.SegmentCounts * max(1, n))()
    rc = K.lib().ts_scan_segments_blocks(tel._ctx.ptr, arr, n, out, cnt)
    assert rc == K.TS_OK, tel._ctx.error()
    res = [ta.SegmentData(out[i], bool(specs[i][2])) for i in range(n)]
    K.lib().ts_free_segments(out, n)
    for k in keep:
        if hasattr(k, "free"):
            k.free()
    return res, [(c.n_windows, c.n_matches, c.n_canonical, c.n_forward) for c in cnt[:n]]


def tracks_call(tel, specs, names):
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    keep, n = [], len(specs)
    arr = segments_in(K, specs, keep)
    out, cnt = (K.SegmentOut * max(1, n))(), (K.SegmentCounts * max(1, n))()
    text = K.TrackText()
    cnames = (C.c_char_p * max(1, n))(*names)
    rc = K.lib().ts_scan_segments_tracks(tel._ctx.ptr, arr, n, cnames, out, cnt, C.byref(text))
    assert rc == K.TS_OK, tel._ctx.error()
    assert all(not out[i].windows and out[i].n_windows == 0 for i in range(n))
    res = [ta.SegmentData(out[i], bool(specs[i][2])) for i in range(n)]
    K.lib().ts_free_segments(out, n)
    got, lines = T.take_text(K, text), int(text.n_lines)
    K.lib().ts_free_track_text(C.byref(text))
    for k in keep:
        if hasattr(k, "free"):
            k.free()
    return res, [(c.n_windows, c.n_matches, c.n_canonical, c.n_forward) for c in cnt[:n]], got, lines


def compare(tel, specs, names, flags=(1, 1, 1)):
    want_res, want_cnt = blocks_call(tel, specs)
    res, cnt, got, lines = tracks_call(tel, specs, names)
    assert cnt == want_cnt
    for g, e in zip(res, want_res):
        assert g.terminalBlocks.tobytes() == e.terminalBlocks.tobytes() and g.interstitialBlocks.tobytes() == e.interstitialBlocks.tobytes()
    want = [b"" if f else None for f in T.track_switches(*flags)]
    n_win = 0
    for sd, name, spec in zip(want_res, names, specs):
        if spec[2]:
            assert len(sd.windows) == 0                             # tips-only: no windows, no lines
            continue
        n_win += len(sd.windows)
        want = [None if a is None else a + b for a, b in zip(want, T.format_windows(name, sd.windows, *flags))]
    assert lines == (n_win if any(flags) else 0)                   # (lines per existing track; no track, no lines)
    for t in range(T.N_TRACKS):
        assert got[t] == want[t], "track %d differs" % t
    return got


def mixed_specs(rng, w, s, on_device):
    lens = [1, w - 1, w, w + 1, w + s, 3 * w + 17, 70_000]
    specs, names, at = [], [], 0
    for i, n in enumerate(lens):
        specs.append((planted(rng, n), at, False, on_device, 1 + 3 * i))
        names.append(b"path%d" % i if i != 3 else b"a_rather_long_sequence_name_of_more_than_sixty_four_bytes_for_the_staging")
        at += n + 5
        if i in (1, 4, 6):                                         # tips-only segments in between: scanned, but no lines
            specs.append((planted(rng, 9000 + i), at, True, on_device, 2))
            names.append(b"tips%d" % i)
            at += 9000 + i
    return specs, names


@pytest.mark.parametrize("on_device", [False, True], ids=["bases", "device"])
@pytest.mark.parametrize("route", ["tiled", "general", "forced general"])
def test_tracks_equal_blocks_plus_reference_text(route, on_device, monkeypatch):
    from teloscope_amd import _capi as K
    if route == "forced general":
        monkeypatch.setenv("TS_FORCE_GENERAL", "1")
    _, tel = make((LIST_FORM if route == "general" else TILED) + " -t 3000")
    monkeypatch.delenv("TS_FORCE_GENERAL", raising=False)
    try:
        assert K.lib().ts_uses_fast_path(tel._ctx.ptr) == (1 if route == "tiled" else 0)
        specs, names = mixed_specs(np.random.default_rng(20261018), 1000, 500, on_device)
        got = compare(tel, specs, names)
        assert got[T.DENSITY].count(b"\n") > 150 and b"\t-1\n" in got[T.STRAND_RATIO]
        assert any(not ln.endswith(b"\t0") for ln in got[T.DENSITY].split(b"\n")[:-1])
    finally:
        tel.close()


def test_only_tips_segments_and_no_segments():
    _, tel = make(TILED)
    try:
        rng = np.random.default_rng(3)
        got = compare(tel, [(planted(rng, 5000), 0, True, False, 0)], [b"t"])
        assert got == [b""] * 5
        got = compare(tel, [], [])
        assert got == [b""] * 5
    finally:
        tel.close()


def test_flags_decide_the_tracks():
    rng = np.random.default_rng(4)
    specs = [(planted(rng, 12_345), 77, False, False, 0)]
    for flags, cli in (((1, 0, 0), "-r"), ((0, 1, 1), "-g -e"), ((0, 0, 0), "")):
        _, tel = make("-w 1000 -s 1000 -i " + cli)
        try:
            got = compare(tel, specs, [b"only"], flags)
            assert [x is None for x in got] == [not f for f in T.track_switches(*flags)]
        finally:
            tel.close()


def test_a_call_that_spans_two_pipeline_groups():
    """Two segments of 140 Mb and one of 10 Mb (a 1 Mb block tiled): the pipeline cuts its groups at ~256 MB of input, so the text
    is appended from more than one group.  w = s = 10 000: 29 000 windows."""
    rng = np.random.default_rng(20261019)
    block = np.frombuffer(planted(rng, 1_000_000), dtype=np.uint8)
    big, small = np.tile(block, 140).tobytes(), np.tile(block, 10).tobytes()
    _, tel = make("-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 10000 -s 10000 -r -g -e")
    try:
        specs = [(big, 0, False, False, 0), (big, 150_000_000, False, False, 0), (small, 300_000_000, False, False, 0)]
        got = compare(tel, specs, [b"chr1", b"chr2", b"chr3"])
        assert got[T.GC].count(b"\n") == 29_000
    finally:
        tel.close()
