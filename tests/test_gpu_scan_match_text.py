"""ts_scan_segments_text against ts_scan_segments on the same segments and context: the text of the two match files equals
tests/matchtext.py applied to the `matches` ts_scan_segments returns (their order included), blocks and counts equal
ts_scan_segments_blocks, no match record and no window record comes back, and window tracks requested beside it equal
ts_scan_segments_tracks — for the tiled kernel with 16- and 32-bit records, the general kernels (a mixed-length set, the tiled
set under TS_FORCE_GENERAL=1), a wide-form set whose stream lies in push order, host and device-resident bases, text pieces,
packed lower-case input, positions above 2^32 and across 10^10, and a call that spans several pipeline groups."""
import ctypes as C

import numpy as np
import pytest

from tests import matchtext as M
from tests import textpieces as TP
from tests import tracktext as T
from tests.test_gpu_input_device import DeviceBytes, make
from tests.test_gpu_scan_tracks import mixed_specs, planted

pytestmark = pytest.mark.gpu

TILED = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -m -i"
LIST_FORM = "-p TTAGGG,TTAGG -w 1000 -s 500 -r -g -e -m -i"
# lengths 6 and 63 under w > s: the wide form, its dense stream written in the reference's push order
WIDE_PUSH = "-c TTAGGG -p TTAGGG," + ("TTAGGG" * 11)[:63] + " -x 0 -w 1000 -s 500 -r -g -e -m -i"
ROUTES = {"tiled": TILED, "tiled rec32": TILED, "list form": LIST_FORM, "forced general": TILED, "wide push order": WIDE_PUSH}


def entries_of(K, specs):
    """test_gpu_scan_tracks' specs (bytes, abs_pos, tips, on_device, shift) -> (format, payload, abs_pos, tips, shift)"""
    return [(K.TS_INPUT_DEVICE if dev else K.TS_INPUT_BASES, seq, a, tips, sh) for seq, a, tips, dev, sh in specs]


class Call:
    """One call's ts_segment_in array; entries: [(format, payload, abs_pos, tips, shift)], payload the bases (TEXT_PIECES: the
    list of a text's pieces)."""

    def __init__(self, tel, entries):
        from teloscope_amd import _capi as K
        self.n = len(entries)
        self.arr, self.keep, self.dev = (K.SegmentIn * max(1, self.n))(), [], []
        for i, (fmt, payload, abs_pos, tips, shift) in enumerate(entries):
            a = self.arr[i]
            if fmt == K.TS_INPUT_TEXT_PIECES:
                pieces = TP.text_pieces(K, payload)
                self.keep.append((payload, pieces))
                a.seq, a.n_pieces, length = C.cast(pieces, C.c_char_p), len(payload), sum(int(p.n_bases) for p in pieces[:len(payload)])
            elif fmt == K.TS_INPUT_PACKED2:
                ps, alive = K.pack_sequence(payload, tel.userInput.foldCase)
                self.keep.append((payload, ps, alive))
                a.seq, length = C.cast(C.pointer(ps), C.c_char_p), len(payload)
            elif fmt == K.TS_INPUT_DEVICE:
                d = DeviceBytes(payload, shift)
                self.dev.append(d)
                a.seq, length = d.ptr, len(payload)
            else:
                self.keep.append(payload)
                a.seq, length = payload, len(payload)
            a.len, a.abs_pos, a.tips_only, a.input_format = length, abs_pos, int(tips), fmt

    def free(self):
        for d in self.dev:
            d.free()


def run(tel, entries, names, what, want_tracks=True, want_matches=True):
    """what: 'matches' (ts_scan_segments), 'blocks', 'tracks' or 'text' -> dict of what came back"""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    call, n = Call(tel, entries), len(entries)
    out, cnt = (K.SegmentOut * max(1, n))(), (K.SegmentCounts * max(1, n))()
    tracks, mtext = K.TrackText(), K.MatchText()
    cnames = (C.c_char_p * max(1, n))(*names)
    lib, ctx = K.lib(), tel._ctx.ptr
    try:
        if what == "matches":
            rc = lib.ts_scan_segments(ctx, call.arr, n, out)
        elif what == "blocks":
            rc = lib.ts_scan_segments_blocks(ctx, call.arr, n, out, cnt)
        elif what == "tracks":
            rc = lib.ts_scan_segments_tracks(ctx, call.arr, n, cnames, out, cnt, C.byref(tracks))
        else:
            rc = lib.ts_scan_segments_text(ctx, call.arr, n, cnames, out, cnt, C.byref(tracks) if want_tracks else None,
                                           C.byref(mtext) if want_matches else None)
        assert rc == K.TS_OK, tel._ctx.error()
        if what in ("tracks", "text"):
            assert all(not out[i].windows and out[i].n_windows == 0 for i in range(n))
        if what != "matches":
            assert all(not out[i].matches and out[i].n_matches == 0 for i in range(n))
        res = dict(segs=[ta.SegmentData(out[i], bool(entries[i][3])) for i in range(n)],
                   counts=[(c.n_windows, c.n_matches, c.n_canonical, c.n_forward) for c in cnt[:n]],
                   tracks=T.take_text(K, tracks), track_lines=int(tracks.n_lines),
                   text=M.take_text(K, mtext), lines=[int(mtext.n_lines[f]) for f in range(M.N_FILES)])
        lib.ts_free_segments(out, n)
        return res
    finally:
        lib.ts_free_track_text(C.byref(tracks))
        lib.ts_free_match_text(C.byref(mtext))
        call.free()


def reference_text(matches, entries, names, bases, limit):
    """tests/matchtext.py over the matches ts_scan_segments returned, segment by segment in input order"""
    want, lines = [b"", b""], [0, 0]
    for sd, (_, _, abs_pos, tips, _), name, seq in zip(matches, entries, names, bases):
        if tips:
            continue
        m = sd._m
        # (only the records that can give a line go through the Python loop: canonical ones, and the others near an end)
        rel = m["position"].astype(np.int64) - abs_pos
        near = (rel <= limit) | (rel >= max(len(seq) - limit, 0))
        sel = m[((m["flags"] & M.MATCH_CANONICAL) != 0) | near]
        text, n = M.format_scanned(name, sel, abs_pos, seq, limit)
        want = [a + b for a, b in zip(want, text)]
        lines = [a + b for a, b in zip(lines, n)]
    return want, lines


def compare(tel, entries, names, bases, limit):
    from teloscope_amd import _capi as K
    stats0 = (C.c_uint64 * 4)()
    stats1 = (C.c_uint64 * 4)()
    matches = run(tel, entries, names, "matches")
    blocks = run(tel, entries, names, "blocks")
    tracks = run(tel, entries, names, "tracks")
    K.lib().ts_match_text_stats(tel._ctx.ptr, stats0)
    got = run(tel, entries, names, "text")
    K.lib().ts_match_text_stats(tel._ctx.ptr, stats1)
    want, want_lines = reference_text(matches["segs"], entries, names, bases, limit)
    assert got["lines"] == want_lines
    for f in range(M.N_FILES):
        assert got["text"][f] == want[f], "match file %d differs" % f
    assert got["counts"] == blocks["counts"]
    for g, e in zip(got["segs"], blocks["segs"]):
        assert g.terminalBlocks.tobytes() == e.terminalBlocks.tobytes() and g.interstitialBlocks.tobytes() == e.interstitialBlocks.tobytes()
    assert got["tracks"] == tracks["tracks"] and got["track_lines"] == tracks["track_lines"]
    assert stats1[1] - stats0[1] == want_lines[0] and stats1[2] - stats0[2] == want_lines[1]
    # either text by itself
    only = run(tel, entries, names, "text", want_tracks=False)
    assert only["text"] == got["text"] and only["tracks"] == [None] * T.N_TRACKS
    only = run(tel, entries, names, "text", want_matches=False)
    assert only["tracks"] == got["tracks"] and only["text"] == [None, None]
    return got, int(stats1[0] - stats0[0])


def make_route(route, monkeypatch, extra=" -t 3000"):
    from teloscope_amd import _capi as K
    if route == "forced general":
        monkeypatch.setenv("TS_FORCE_GENERAL", "1")
    if route == "tiled rec32":
        monkeypatch.setenv("TS_REC32", "1")
    opts, tel = make(ROUTES[route] + extra)
    monkeypatch.delenv("TS_FORCE_GENERAL", raising=False)
    monkeypatch.delenv("TS_REC32", raising=False)
    assert K.lib().ts_uses_fast_path(tel._ctx.ptr) == (1 if route.startswith("tiled") else 0)
    return opts, tel


@pytest.mark.parametrize("on_device", [False, True], ids=["bases", "device"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_text_equals_the_reference_over_the_scans_matches(route, on_device, monkeypatch):
    from teloscope_amd import _capi as K
    opts, tel = make_route(route, monkeypatch)
    try:
        rng = np.random.default_rng(20261019)
        specs, names = mixed_specs(rng, 1000, 500, on_device)
        if route == "wide push order":                              # 63-base matches for the long pattern, across a window's end
            seq = bytearray(specs[-2][0] if specs[-1][2] else specs[-1][0])
            i = len(specs) - 2 if specs[-1][2] else len(specs) - 1
            for at in (1500, 4990, 5460, 20_470, 40_955):             # (the first inside the terminal zone)
                seq[at:at + 126] = b"TTAGGG" * 21
            specs[i] = (bytes(seq),) + specs[i][1:]
        entries = entries_of(K, specs)
        got, _ = compare(tel, entries, names, [s[0] for s in specs], opts.terminal_limit)
        assert got["lines"][0] > 300 and got["lines"][1] > (0 if route in ("list form", "wide push order") else 10)
        assert b"a_rather_long_sequence_name" in got["text"][0]
    finally:
        tel.close()


def test_text_pieces_and_packed_lower_case_input(monkeypatch):
    from teloscope_amd import _capi as K
    opts, tel = make_route("tiled", monkeypatch)
    try:
        rng = np.random.default_rng(7)
        a, b, c = planted(rng, 70_000), planted(rng, 33_333), planted(rng, 5_017)
        text = TP.render(a, 60, "lf", rng, ending=b"\n")
        blobs = TP.split(text, TP.cut_places(text, rng, 5))
        entries = [(K.TS_INPUT_TEXT_PIECES, blobs, 11, False, 0), (K.TS_INPUT_PACKED2, b.lower(), 80_000, False, 0),
                   (K.TS_INPUT_PACKED2, c.lower(), 120_000, True, 0), (K.TS_INPUT_BASES, c.lower(), 130_000, False, 0)]
        got, _ = compare(tel, entries, [b"pieces", b"packed", b"tips", b"lower"], [a, b.lower(), c.lower(), c.lower()], opts.terminal_limit)
        assert got["lines"][0] > 300 and b"packed\t" in got["text"][0] and b"lower\t" in got["text"][0]
        assert all(ln.split(b"\t")[3].isupper() for ln in (got["text"][0] + got["text"][1]).splitlines())
    finally:
        tel.close()


@pytest.mark.parametrize("route", ["tiled", "list form"])
def test_positions_above_2_32_and_across_10_10(route, monkeypatch):
    from teloscope_amd import _capi as K
    opts, tel = make_route(route, monkeypatch)
    try:
        rng = np.random.default_rng(11)
        seqs = [planted(rng, 9_000), planted(rng, 3_000), planted(rng, 4_001)]
        at = [(1 << 32) + 12_345, 10 ** 10 - 600, (1 << 40) + 7]
        entries = [(K.TS_INPUT_BASES, s, p, False, 0) for s, p in zip(seqs, at)]
        got, _ = compare(tel, entries, [b"big%d" % i for i in range(3)], seqs, opts.terminal_limit)
        assert b"big1\t99999999" in got["text"][0] and b"big1\t10000000" in got["text"][0] and b"big2\t10995116" in got["text"][0]
    finally:
        tel.close()


def test_only_tips_segments_and_no_segments(monkeypatch):
    from teloscope_amd import _capi as K
    opts, tel = make_route("tiled", monkeypatch)
    try:
        rng = np.random.default_rng(3)
        s = planted(rng, 5000)
        got, calls = compare(tel, [(K.TS_INPUT_BASES, s, 0, True, 0)], [b"t"], [s], opts.terminal_limit)
        assert got["text"] == [b"", b""] and got["lines"] == [0, 0]
        got, _ = compare(tel, [], [], [], opts.terminal_limit)
        assert got["text"] == [b"", b""]
    finally:
        tel.close()


def test_a_context_without_m_gives_tracks_and_no_match_text():
    from teloscope_amd import _capi as K
    _, tel = make("-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -i -t 3000")
    try:
        rng = np.random.default_rng(5)
        s = planted(rng, 20_000)
        entries = [(K.TS_INPUT_BASES, s, 0, False, 0)]
        got = run(tel, entries, [b"x"], "text")
        assert got["text"] == [None, None] and got["lines"] == [0, 0]
        assert got["tracks"] == run(tel, entries, [b"x"], "tracks")["tracks"] and got["track_lines"] == 40
    finally:
        tel.close()


def test_a_call_that_spans_pipeline_groups():
    """Four segments of 140 Mb and one of 10 Mb (a 1 Mb block tiled): the pipeline cuts its groups at 256 or 512 MB of input, so
    the text is appended from more than one group, each formatted from its own records and its own input buffer."""
    from teloscope_amd import _capi as K
    rng = np.random.default_rng(20261019)
    block = np.frombuffer(planted(rng, 1_000_000), dtype=np.uint8)
    big, small = np.tile(block, 140).tobytes(), np.tile(block, 10).tobytes()
    opts, tel = make("-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 10000 -s 10000 -r -g -e -m")
    try:
        seqs = [big, big, big, big, small]
        entries = [(K.TS_INPUT_BASES, s, 150_000_000 * i, False, 0) for i, s in enumerate(seqs)]
        names = [b"chr%d" % (i + 1) for i in range(5)]
        matches = run(tel, entries, names, "matches")
        st0, st1 = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
        K.lib().ts_match_text_stats(tel._ctx.ptr, st0)
        got = run(tel, entries, names, "text")
        K.lib().ts_match_text_stats(tel._ctx.ptr, st1)
        want, want_lines = reference_text(matches["segs"], entries, names, seqs, opts.terminal_limit)
        assert got["lines"] == want_lines and want_lines[0] > 100_000 and want_lines[1] > 0
        assert got["text"] == want
        assert got["tracks"][T.GC].count(b"\n") == 57_000
        assert st1[0] - st0[0] >= 2                                  # one formatting call per group
        assert [c[2] for c in got["counts"]] == [len(sd.canonicalMatches) for sd in matches["segs"]]
    finally:
        tel.close()
