"""The packed upload (pipeline.cpp: upload_pieces, pack.cpp, unpack.hip) where the suite did not reach it: FASTA text packed
straight from the text (ts::pack_text), blocks that mix pieces and formats, the staging workers' range cuts, and chunks that
begin anywhere in a 64-position line of the layout.  Every result is compared record for record with the oracle on the joined
bases and with the same call on the plain route (TS_PACKED_UPLOAD=0); ts_upload_stats says that the path under test ran."""
import numpy as np
import pytest

from tests import harness as H
from tests import seqgen
from tests import textpieces as T
from tests.backends import OracleBackend, assert_segment_equal

pytestmark = pytest.mark.gpu

TILED = "-w 1000 -s 500 -r -g -e -m -i"
GENERAL = "-p TTAGGG,TTAGG -w 1000 -s 500 -r -g -e -m -i"
SETS = {"tiled": TILED, "general": GENERAL}
PACKED, ASCII, PLAIN_BLOCKS, TEXT_BLOCKS, COPIED_BLOCKS, MIXED_BLOCKS, MULTI_WORKER, OFF_BOUNDARY = range(8)


def make(cli, fold=True):
    import teloscope_amd as ta
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("x.fa " + cli)
    ui = user_input(opts, device=0)
    ui.foldCase = fold
    return opts, ta.Teloscope(ui)


def route(tel, monkeypatch, packed):
    monkeypatch.setenv("TS_PACKED_UPLOAD", "1" if packed else "0")
    monkeypatch.setenv("TS_PACKED_MIN_BYTES", "0")
    tel._ctx.refresh_env()                                         # (the context read its knobs when it was made)


def stats_of(tel, call):
    before = tel.upload_stats()
    res = call()
    return res, tuple(a - b for a, b in zip(tel.upload_stats(), before))


def device_bytes(data):
    from tests.test_gpu_input_device import DeviceBytes
    return DeviceBytes(data, 3)


def spoil(rng, n, at=(), soft=2):
    """A chromosome of n bases with IUPAC codes, soft-masked stretches and an invalid run of 2 to 9 bases (N, n or IUPAC)
    laid across every position of `at`."""
    s = bytearray(seqgen.chromosome(rng, n, telo_repeats=min(150, max(1, n // 40)), tvr_rate=0.03, n_its=3, iupac=n // 3000))
    for _ in range(soft if n > 2000 else 0):
        a, ln = int(rng.integers(0, n - 700)), int(rng.integers(40, 700))
        s[a:a + ln] = bytes(s[a:a + ln]).lower()
    for p in at:
        ln = int(rng.integers(2, 10))
        a = max(0, min(n - ln, int(p) - int(rng.integers(1, ln))))
        s[a:a + ln] = bytes(b"NnRY"[int(rng.integers(0, 4))] for _ in range(ln)) if ln & 1 else b"N" * ln
    return bytes(s)


def check(got, exp, entries, what):
    for i, (g, e) in enumerate(zip(got, exp)):
        assert_segment_equal(g, e, bool(entries[i][3]), ctx="%s segment %d" % (what, i))


# ------------------------------------------------------------------------------------------------------------ a: text forms
TEXT_LENGTHS = [4096, 4097, 16383, 16385, 33333, 36001, 40001, 45003, 49153, 57005, 70001]
TEXT_WIDTHS = [1, 31, 2, 60, 33, 64, 80, 32, 63, 65, 70]             # each of the eleven once; the long segments get the usual ones
WHOLE_BLOCKS = 2 * 16384 + 64                                        # bases that hold a whole 16384-block wherever the piece lies


def text_entries(K, rng):
    """Eleven segments of 4096 to 70 001 bases as text pieces: each of the eleven line widths once, the four line-end styles in
    turn, a first line that ends in bytes 30 to 33 of a 32-byte round, pieces cut inside lines, before line ends, between CR and
    LF and behind LF, invalid runs across line ends, piece ends and the 16384-blocks of the layout (the segments lie at 16-byte
    multiples of it, so runs are laid every 1024 bases too).  The segments of 33 333 bases and more are cut only behind their
    first 32 832 bases, so each of their widths has a block packed straight from the text; the four short ones are cut all over
    and have mixed blocks only."""
    entries, bases = [], []
    assert sorted(TEXT_WIDTHS) == sorted(T.WIDTHS) and len(TEXT_WIDTHS) == len(TEXT_LENGTHS)
    for i, (n, width) in enumerate(zip(TEXT_LENGTHS, TEXT_WIDTHS)):
        style, keep = T.STYLES[i % len(T.STYLES)], WHOLE_BLOCKS if n >= 33333 else 0
        near = [int(x) for x in rng.integers(keep + 100, n - 100, size=6)]
        at = list(range(1024, n, 1024)) + [width * int(k) for k in rng.integers(1, n // width, size=12)] + near
        seq = spoil(rng, n, at)
        text = T.render(seq, width, style, rng, first=(30 + i % 4) if i % 2 else None)
        p0, b0 = T.behind_bases(text, keep) if keep else (0, 0)        # the cuts lie behind the bases to keep in one piece
        cuts = [] if i == 0 else [p0 + p for p in T.cut_places(text[p0:], rng, 3 + 4 * (i % 3), near=[x - b0 for x in near if x > b0])]
        blobs = T.split(text, cuts)
        assert i == 0 or (len(blobs) >= 4 and len(T.to_bases(blobs[0])) >= keep)
        entries.append((K.TS_INPUT_TEXT_PIECES, blobs, 1000 * i + 7, False))
        bases.append(T.to_bases(text))
        if n <= 16385:
            assert bases[-1] == T.to_bases_bytewise(text)          # (the rule as stated, where a byte at a time is affordable)
    # the cuts the generator draws have to include the ones that matter: between a CR and its LF, right behind an LF, right
    # before a line end, and inside a line
    pairs = [(a, b) for _, blobs, _, _ in entries for a, b in zip(blobs, blobs[1:])]
    assert sum(a.endswith(b"\r") and b.startswith(b"\n") for a, b in pairs) >= 3
    assert sum(a.endswith(b"\n") for a, b in pairs) >= 3
    assert sum(b[:1] in b"\r\n" and a[-1:] not in b"\r\n" for a, b in pairs) >= 3
    assert sum(b[:1] not in b"\r\n" and a[-1:] not in b"\r\n" for a, b in pairs) >= 3
    return entries, bases


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", sorted(SETS))
def test_text_pieces_packed_from_the_text(name, fold, monkeypatch):
    from teloscope_amd import _capi as K
    opts, tel = make(SETS[name], fold)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(20261018 + int(fold))
    entries, bases = text_entries(K, rng)
    assert any(b"\r" in b for b in bases) and sum(len(e[1]) > 1 for e in entries) >= 9
    exp = [orac.scan_segment(b.upper() if fold else b, ap, False) for b, (_, _, ap, _) in zip(bases, entries)]
    route(tel, monkeypatch, True)
    got, st = stats_of(tel, lambda: T.scan_call(tel, entries))
    check(got, exp, entries, "text pieces, packed route")
    assert st[PACKED] > 0 and st[ASCII] == 0 and st[TEXT_BLOCKS] >= 7 and st[MIXED_BLOCKS] > 0, "the path under test did not run: %r" % (st,)
    # the same text as joined bases, and through the plain route
    joined = [(K.TS_INPUT_BASES, b, ap, False) for b, (_, _, ap, _) in zip(bases, entries)]
    check(T.scan_call(tel, joined), exp, entries, "joined bases, packed route")
    route(tel, monkeypatch, False)
    got, st = stats_of(tel, lambda: T.scan_call(tel, entries))
    check(got, exp, entries, "text pieces, plain route")
    assert st[PACKED] == 0 and st[ASCII] > 0
    # a text that holds fewer bases than its piece declares: an error on the packed route too
    route(tel, monkeypatch, True)
    blobs = entries[3][1]
    pieces = T.text_pieces(K, blobs)
    pieces[len(blobs) - 1].n_bases += 5
    short = (K.TS_INPUT_TEXT_PIECES, (blobs, len(bases[3]) + 5, pieces), 0, False)
    rc, st = stats_of(tel, lambda: T.scan_call(tel, [entries[1], short], raw=True))
    assert rc == K.TS_ERR_INVALID_ARG and st[PACKED] > 0
    check(T.scan_call(tel, entries[:2]), exp[:2], entries, "after the refused call")


# ------------------------------------------------------------------------------------------------- b: mixed formats in one call
_MIXED = {}


def mixed_segments():
    """Sixty sequences of 1 to 40 000 bases, the same for every phase and parameter set."""
    if "seqs" not in _MIXED:
        rng = np.random.default_rng(77)
        lengths = [1, 2, 3, 5, 63, 64, 65, 300, 4095, 4097] + [int(x) for x in rng.integers(1, 40001, size=42)]
        lengths = [lengths[j] for j in rng.permutation(len(lengths))]
        for at in (9, 30):                                         # four of 40 000 in a row, twice: one of every format whatever the phase,
            lengths[at:at] = [40000] * 4                           # each long enough to hold whole blocks of 16384
        _MIXED["seqs"] = [spoil(rng, n, at=[0, n // 2, n] if n > 40 else [], soft=1) for n in lengths]
    return _MIXED["seqs"]


def mixed_expected(name, opts):
    """The oracle's results for them, computed once per parameter set."""
    if name not in _MIXED:
        orac = OracleBackend(opts)
        _MIXED[name] = [orac.scan_segment(seq.upper(), 100 * i, False) for i, seq in enumerate(mixed_segments())]
    return _MIXED[name]


@pytest.mark.parametrize("phase", range(4))
@pytest.mark.parametrize("name", sorted(SETS))
def test_formats_mixed_in_one_call(name, phase, monkeypatch):
    """Sixty segments of 1 to 40 000 bases whose formats cycle through BASES, TEXT_PIECES, PACKED2 and DEVICE from each of the
    four phases: the 16384-blocks at the seams spell packed codes out as letters next to ASCII and text, blocks inside long
    packed segments copy codes, blocks inside long plain ones pack in place."""
    from teloscope_amd import _capi as K
    opts, tel = make(SETS[name])
    exp = mixed_expected(name, opts)
    rng = np.random.default_rng(phase)                             # (the texts' line ends and cuts)
    formats = [K.TS_INPUT_BASES, K.TS_INPUT_TEXT_PIECES, K.TS_INPUT_PACKED2, K.TS_INPUT_DEVICE]
    entries, plain = [], []
    for i, seq in enumerate(mixed_segments()):
        fmt = formats[(i + phase) % 4]
        if fmt == K.TS_INPUT_TEXT_PIECES:
            text = T.render(seq, T.WIDTHS[i % len(T.WIDTHS)], T.STYLES[i % 3], rng)
            payload = T.split(text, T.cut_places(text, rng, i % 4) if len(seq) > 10 else [])
            assert T.to_bases(text) == seq
        else:
            payload = seq
        entries.append((fmt, payload, 100 * i, False))
        plain.append((K.TS_INPUT_BASES, seq, 100 * i, False))
    route(tel, monkeypatch, True)
    got, st = stats_of(tel, lambda: T.scan_call(tel, entries, device_bytes))
    check(got, exp, entries, "mixed formats, phase %d" % phase)
    assert st[MIXED_BLOCKS] > 0 and st[COPIED_BLOCKS] > 0 and st[PLAIN_BLOCKS] > 0, "the path under test did not run: %r" % (st,)
    check(T.scan_call(tel, plain), exp, plain, "all bases, packed route")
    route(tel, monkeypatch, False)
    check(T.scan_call(tel, entries, device_bytes), exp, entries, "mixed formats, plain route, phase %d" % phase)


# ------------------------------------------------------------------------------------------------------------ c: worker cuts
def test_staging_workers_cut_at_text_pieces(monkeypatch):
    """One call of 9 Mi bases — 8 MiB in all and a chunk of 4 MiB are where the staging pool and its range cuts begin: a 6 Mb
    segment as text pieces of 50 kb to 1.5 Mb (some begin within half a share of an even cut, some do not) and a 3 Mb plain one,
    an invalid run across every multiple of 4096 of the first 2 Mb and across every piece's first base.  Against the plain route
    on everything and the oracle on both segments."""
    import os
    from teloscope_amd import _capi as K
    if len(os.sched_getaffinity(0)) < 4:
        pytest.skip("fewer than four hardware threads: upload_pieces stages with one worker, there are no cuts")
    opts, tel = make(TILED)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(5)
    n_text, n_plain = 6 * 1024 * 1024 + 12345, 3 * 1024 * 1024 + 77
    sizes = [50_000, 1_500_000, 333_333, 70_001, 1_048_576, 786_432 + 5, 1_200_003, 262_144 + 2, 500_000]
    sizes.append(n_text - sum(sizes))
    assert 50_000 <= sizes[-1] <= 1_500_000
    starts = np.cumsum([0] + sizes[:-1])
    seq = spoil(rng, n_text, at=list(range(4096, 2_000_000, 4096)) + [int(s) for s in starts[1:]], soft=30)
    blobs = []
    for k, (a, ln) in enumerate(zip(starts, sizes)):
        # every piece a text of its own; one ends between a CR and its LF, the next begins with that LF
        ending = b"\r" if k == 2 else (b"" if k % 2 else b"\r\n")
        blobs.append((b"\n" if k == 3 else b"") + T.render(seq[a:a + ln], [60, 80, 70][k % 3], ["lf", "crlf", "mix"][k % 3], rng, ending=ending))
    assert b"".join(T.to_bases(b) for b in blobs) == seq
    other = spoil(rng, n_plain, at=[4096, 16384], soft=10)
    entries = [(K.TS_INPUT_TEXT_PIECES, blobs, 11, False), (K.TS_INPUT_BASES, other, 13, False)]
    route(tel, monkeypatch, True)
    got, st = stats_of(tel, lambda: T.scan_call(tel, entries))
    assert st[MULTI_WORKER] > 0 and st[PACKED] > 0 and st[TEXT_BLOCKS] > 0, "the path under test did not run: %r" % (st,)
    route(tel, monkeypatch, False)
    ref = T.scan_call(tel, entries)
    # (the oracle takes a fraction of a second at this size: both routes against it on everything)
    exp = [orac.scan_segment(seq.upper(), 11, False), orac.scan_segment(other.upper(), 13, False)]
    check(got, exp, entries, "packed route against the oracle")
    check(ref, exp, entries, "plain route against the oracle")


# ------------------------------------------------------------------------------- d: chunk starts and destination alignment
def tip_contigs(tel, t, n=128):
    """n contigs of about 140 000 bases for a tips-only scan with terminal regions of t bases: every contig's second region is a
    chunk (the gap in front of it exceeds 64 KiB; the next contig's first region rides along), and those regions' layout offsets cover all 64 residues modulo 64
    (asserted: it is what the test is about), so the unpack kernel meets every chunk start within a 64-position line and every
    destination alignment within 16 bytes."""
    from teloscope_amd.distributed import ShardPlan
    # (lengths 140 000 + i leave residues out: segments lie at multiples of 16 of the layout; so contig i takes the length from
    # 140 000 on that puts its second region on residue i modulo 64, given that rule — the plan below has the last word)
    lens, off = [], 0
    for i in range(n):
        lens.append(140_000 + (i % 64 - (off + 140_000 - t)) % 64)
        off = (off + lens[-1] + 15) // 16 * 16
    plan = ShardPlan(tel, lens, tips_only=True, world=1)
    offs = plan.segment_offsets()
    plan.close()
    second = [o + ln - t for o, ln in zip(offs, lens)]
    assert {x % 64 for x in second} == set(range(64)), sorted({x % 64 for x in second})
    assert all(b - (a + t) > 65536 for a, b in zip(offs, second))
    return lens


@pytest.mark.parametrize("cli,t", [("-t 300", 300), ("-t 4100", 4100)])
def test_chunks_that_begin_anywhere_in_a_line_of_the_layout(cli, t, monkeypatch):
    """-t 300: as TS_INPUT_PACKED2 every region is a packed chunk (bases that arrive packed leave packed), as TS_INPUT_BASES a
    region of 300 bases is below the 4096 a packed chunk takes and goes as ASCII — asserted, so that nobody reads the BASES
    run as a test of the unpack kernel; -t 4100 is the smallest round length at which the BASES regions are packed too.  Each
    region carries an invalid run within its first 20 and one within its last 20 bases: the byte-wise end groups of
    ts_unpack_bases and ts_poke_invalid write the same 16-byte lines."""
    from teloscope_amd import _capi as K
    opts, tel = make(cli)
    orac = OracleBackend(opts)
    rng = np.random.default_rng(t)
    seqs = []
    for i, n in enumerate(tip_contigs(tel, t)):
        s = bytearray(seqgen.chromosome(rng, n, telo_repeats=100, tvr_rate=0.03, n_its=1, iupac=20))
        for lo, hi in ((0, t), (n - t, n)):
            a, b = lo + i % 17, hi - 1 - i % 13                  # the first of the first 20, the last of the last 20
            s[a:a + 2 + i % 5] = b"N" * (2 + i % 5)
            s[b - (1 + i % 7):b + 1] = b"n" * (2 + i % 7)
        if i % 3 == 0:
            s[0:1], s[n - 1:n] = b"N", b"R"                       # the region's very first and very last base
        seqs.append(bytes(s))
    exp = [orac.scan_segment(s.upper(), 10 * i, True) for i, s in enumerate(seqs)]
    as_bases = [(K.TS_INPUT_BASES, s, 10 * i, True) for i, s in enumerate(seqs)]
    as_packed = [(K.TS_INPUT_PACKED2, s, 10 * i, True) for i, s in enumerate(seqs)]
    route(tel, monkeypatch, True)
    got, st = stats_of(tel, lambda: T.scan_call(tel, as_packed))
    check(got, exp, as_packed, "packed in, %s" % cli)
    assert st[OFF_BOUNDARY] >= 63 and st[PACKED] >= len(seqs), "the path under test did not run: %r" % (st,)
    got, st = stats_of(tel, lambda: T.scan_call(tel, as_bases))
    check(got, exp, as_bases, "bases in, %s" % cli)
    if t >= 4096:
        assert st[OFF_BOUNDARY] >= 63 and st[ASCII] == 0, "the path under test did not run: %r" % (st,)
    else:
        assert st[PACKED] == 0 and st[ASCII] >= len(seqs), st
    route(tel, monkeypatch, False)
    check(T.scan_call(tel, as_bases), exp, as_bases, "bases in, plain route, %s" % cli)
