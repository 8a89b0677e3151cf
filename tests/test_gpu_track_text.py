"""The device track formatter by itself: ts_window_tracks_format (teloscope_amd/csrc/tracks.hip, tracks.cpp) through ctypes, every
track compared byte for byte with the plain-Python reference tests/tracktext.py (which tests/test_track_format_core_cpu.py pins
against the writer's restatement and against printf).  Records are handmade, so that values no small scan produces are
formatted: ties, the exponent form, -1, empty windows, short trailing windows of every size.  Every call is small."""
import numpy as np
import pytest

from tests import tracktext as T
from tests.test_gpu_input_device import make

pytestmark = pytest.mark.gpu

BLOCK = 256                    # windows per workgroup (TS_TRACK_BLOCK, ts_internal.h)
SLICE = 1 << 21                # windows per pass (kSliceWindows, tracks.cpp)
WS = [(1000, 500), (1024, 1024), (7, 3), (4096, 4096), (4194304, 4194304)]
FLAGS = {"r": (1, 0, 0), "g": (0, 1, 0), "e": (0, 0, 1), "rge": (1, 1, 1)}


def context(w, s, flags):
    r, g, e = flags
    return make("-w %d -s %d%s%s%s" % (w, s, " -r" * r, " -g" * g, " -e" * e))[1]


def random_records(rng, sizes):
    """a record per window size: nucleotide counts that sum to at most the size, covered counts at most the size"""
    out = np.zeros((len(sizes), 8), dtype=np.uint32)
    for i, size in enumerate(sizes):
        cuts = np.sort(rng.integers(0, size + 1, size=4))
        out[i, :4] = [cuts[0], cuts[1] - cuts[0], cuts[2] - cuts[1], cuts[3] - cuts[2]]
        fwd = int(rng.integers(0, size + 1))
        rev = int(rng.integers(0, size - fwd + 1))
        can = int(rng.integers(0, fwd + rev + 1))
        out[i, 4:] = [can, fwd + rev - can, fwd, rev]
    return out


def special_records(w, size):
    """records of a window of `size` bases that reach the formatter's corners"""
    recs = [
        [1, 2, 3, 1, 0, 0, 0, 0],                               # nothing covered: density 0, both ratios -1
        [0, 0, 0, 0, 0, 0, 0, 0],                               # an all-N window: entropy 0, GC 0
        [0, 0, 0, 0, size, 0, size, 0],                         # ratios equal to 1, density 1
        [size, 0, 0, 0, 0, size, 0, size],                      # one count equal to the size; ratios 0
        [0, size, 0, 0, 1, 0, 1, 0],                            # GC 100; covered = 1 (w = 2^22: 2.38419e-07)
        [0, 0, size, 0, 1, 1023, 1, 2],                         # canonical ratio 1 / 1024, a tie: 0.000976562
        [0, 0, 0, size, 3, 4093, 3, 0],                         # canonical ratio 3 / 4096, a tie; density 3 / 4096 at w = 4096
        [size // 4, size // 4, size // 4, size // 4, 1, 2, 2, 1],
    ]
    return [[min(x, 0xFFFFFFFF) for x in r] for r in recs if max(r[:4]) <= size]


def seg_sizes(length, w, s):
    return [min(w, length - k * s) for k in range(T.n_windows(length, s))]


def layout(lens, s, abs_pos=0, names=None):
    """segments of the given lengths back to back (17 bases apart) -> the segment table"""
    segs, first, at = [], 0, abs_pos
    for i, ln in enumerate(lens):
        n = T.n_windows(ln, s)
        segs.append((first, n, at, ln, names[i] if names else b"chr%d" % (i + 1)))
        first += n
        at += ln + 17
    return segs


def check(tel, records, segs, w, s, flags, want=None):
    got, n_lines = T.device_format(tel, records, segs)
    want = T.format_tracks(records, segs, w, s, *flags) if want is None else want
    assert [x is None for x in got] == [x is None for x in want]              # a disabled track: NULL, length 0
    for t in range(T.N_TRACKS):
        assert got[t] == want[t], "track %d differs" % t
    assert n_lines == sum(sg[1] for sg in segs)
    return got


@pytest.fixture(scope="module")
def per_ws():
    """Per (w, s): one case with every special record, random records and trailing short windows, and its reference text with
    all tracks on — the contexts with one flag take their tracks from it."""
    out = {}
    for w, s in WS:
        rng = np.random.default_rng(w * 31 + s)
        lens = [0, 3 * w + 17, 1, w - 1, 0, 0, w, w + 1, w + s] + ([k for k in range(1, w)] if w == 7 else [w // 3 * 2, w // 7 + 1, 999 % w + 1])
        lens += [(len(special_records(w, w)) + w // s) * s, 0]        # (its first windows are full ones: the special records' place)
        segs = layout(lens, s, abs_pos=max(0, 9_999_000 - 2 * w))         # (the start gains a digit inside the second segment)
        sizes = [x for ln in lens for x in seg_sizes(ln, w, s)]
        records = random_records(rng, sizes)
        sp = special_records(w, w)
        first = segs[-2][0]
        for j, r in enumerate(sp):
            if sizes[first + j] == w:
                records[first + j] = r
        for j, r in enumerate(special_records(w, sizes[1])[:2]):  # ... and on full windows of the first real segment
            records[1 + j] = r
        out[(w, s)] = (records, segs, T.format_tracks(records, segs, w, s, 1, 1, 1))
    return out


@pytest.mark.parametrize("flag", sorted(FLAGS))
@pytest.mark.parametrize("w,s", WS)
def test_contexts_and_special_records(per_ws, w, s, flag):
    records, segs, full = per_ws[(w, s)]
    flags = FLAGS[flag]
    on = T.track_switches(*flags)
    tel = context(w, s, flags)
    try:
        got = check(tel, records, segs, w, s, flags, [full[t] if on[t] else None for t in range(T.N_TRACKS)])
    finally:
        tel.close()
    if flag == "rge":
        assert b"\t-1\n" in got[T.CANON_RATIO] and b"\t-1\n" in got[T.STRAND_RATIO] and b"\t0\n" in got[T.DENSITY]
        assert b"\t0.000976562\n" in got[T.CANON_RATIO] and b"\t0.000732422\n" in got[T.CANON_RATIO]
        assert b"\t100\n" in got[T.GC] and b"\t0\n" in got[T.ENTROPY] and (w % 4 or b"\t2\n" in got[T.ENTROPY])
        if w == 4194304:
            assert b"\t2.38419e-07\n" in got[T.DENSITY]
        if w == 4096:
            assert b"\t0.000732422\n" in got[T.DENSITY]


@pytest.fixture(scope="module")
def tel_1000():
    tel = context(1000, 500, (1, 1, 1))
    yield tel
    tel.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 4097])
def test_window_counts_around_waves_and_workgroups(tel_1000, n):
    rng = np.random.default_rng(n)
    length = (n - 1) * 500 + 333 if n else 0
    segs = layout([length], 500, abs_pos=99_000)
    records = random_records(rng, seg_sizes(length, 1000, 500))
    assert len(records) == n
    check(tel_1000, records, segs, 1000, 500, (1, 1, 1))


def test_seventy_thousand_windows(tel_1000):
    rng = np.random.default_rng(70000)
    length = 70_000 * 500                                          # (the last window holds 500 bases)
    segs = layout([length], 500)
    base = random_records(rng, [1000] * 997)                       # (997 distinct records, repeated: the reference memoises)
    records = base[np.arange(70_000) % 997]
    records[-1] = [500, 0, 0, 0, 7, 0, 7, 0]
    check(tel_1000, records, segs, 1000, 500, (1, 1, 1))


def test_more_windows_than_one_pass_takes():
    """2^21 + 1 windows: the formatter works through the records in passes of 2^21; the GC track alone, whose text is cheap to
    restate (four distinct values)."""
    w = s = 100
    n = SLICE + 1
    tel = context(w, s, (0, 1, 0))
    try:
        records = np.zeros((n, 8), dtype=np.uint32)
        records[:, 1] = np.arange(n) % 4 * 25
        segs = [(0, n, 0, n * w, b"c")]
        val = [b"0", b"25", b"50", b"75"]
        want = b"".join([b"c\t%d\t%d\t%s\n" % (k * w, k * w + w, val[k & 3]) for k in range(n)])
        got, n_lines = T.device_format(tel, records, segs)
        assert got[T.GC] == want and n_lines == n
        assert [x is None for x in got] == [True, True, True, False, True]
    finally:
        tel.close()


def test_segment_layouts(tel_1000):
    w, s = 1000, 500
    one_window = [1 + (i * 37) % s for i in range(700)]           # every lane of a wave and of a workgroup in another segment
    mixed = [bytes(97 + (i + k) % 26 for k in range(1 + (i * 11) % 90)) for i in range(700)]
    for lens, names in (([40_000], None), ([700] * 300, None), ([500] * 300, None), (one_window, mixed), ([0, 2000, 0, 0, 1500, 0, 1, 0], None),
                        ([0, 0, 0], None), ([5000, 0, 5000], None), ([5000, 5000, 0], None)):
        rng = np.random.default_rng(len(lens))
        segs = layout(lens, s, names=names)
        if lens[0] in (500, 1):
            assert all(sg[1] == 1 for sg in segs)                  # 300 (700) segments of one window each
        records = random_records(rng, [x for ln in lens for x in seg_sizes(ln, w, s)])
        check(tel_1000, records, segs, w, s, (1, 1, 1))


@pytest.mark.parametrize("abs_pos", [0, 9_999_000, 2 ** 32 - 700, 10 ** 15])
def test_absolute_positions(tel_1000, abs_pos):
    w, s = 1000, 500
    rng = np.random.default_rng(abs_pos % 1000)
    lens = [2600, 130 * s + 1]
    segs = layout(lens, s, abs_pos=abs_pos)
    records = random_records(rng, [x for ln in lens for x in seg_sizes(ln, w, s)])
    got = check(tel_1000, records, segs, w, s, (1, 1, 1))
    if abs_pos == 2 ** 32 - 700:
        assert b"\t4294967096\t4294968096\t" in got[T.GC]         # a window across 2^32


def test_name_lengths(tel_1000):
    """Names of 1, 7, 63, 64, 65 and 300 bytes (with 300, a wave's 64 lines exceed the staging area: the bytewise path), and
    every length from 1 to 70 in one call, three windows each, so that lines of changing length cross waves and 16-byte lines."""
    w, s = 1000, 500
    rng = np.random.default_rng(5)
    for n in (1, 7, 63, 64, 65, 300):
        lens = [100 * s]
        segs = layout(lens, s, names=[bytes(65 + (i * 7) % 26 for i in range(n))])
        records = random_records(rng, seg_sizes(lens[0], w, s))
        check(tel_1000, records, segs, w, s, (1, 1, 1))
    lens = [3 * s] * 70
    segs = layout(lens, s, names=[bytes(97 + (i + k) % 26 for k in range(i + 1)) for i in range(70)])
    records = random_records(rng, [x for ln in lens for x in seg_sizes(ln, w, s)])
    check(tel_1000, records, segs, w, s, (1, 1, 1))
    lens = [70 * s, 3 * s, 70 * s]                                 # a long name between short ones within one workgroup
    segs = layout(lens, s, names=[b"a", b"L" * 300, b"b"])
    records = random_records(rng, [x for ln in lens for x in seg_sizes(ln, w, s)])
    check(tel_1000, records, segs, w, s, (1, 1, 1))


def test_device_floats_bit_for_bit_over_all_ratios():
    """Every n / d with d <= 1024 as density (covered / size), canonical ratio and GC, formatted by the device and compared as
    text with the reference's float32 division: the test an approximate division fails.  w = 1024, s = 1: a segment of 1024 bases
    has windows of 1024, 1023, ... bases; segment j carries n = j in its windows of at least j bases."""
    w, s = 1024, 1
    tel = context(w, s, (1, 1, 0))
    try:
        segs, recs, want, first = [], [], [[], [], []], 0
        f32 = np.float32
        text = {}
        for j in range(0, w + 1):
            n_win = w - max(j, 1) + 1
            segs.append((first, n_win, 0, w, b"s"))
            first += n_win
            d = w - np.arange(n_win)
            r = np.zeros((n_win, 8), dtype=np.uint32)
            r[:, 1] = j                                             # GC count
            r[:, 4], r[:, 5], r[:, 6] = j, d - j, j                 # canonical, non-canonical, forward
            recs.append(r)
            for dd in d:
                dd = int(dd)
                if (j, dd) not in text:
                    q = f32(j) / f32(dd)
                    text[(j, dd)] = (b"%g" % float(q), b"%g" % float(f32(float(q) * 100.0)))
                ratio, gc = text[(j, dd)]
                want[0].append(ratio)
                want[1].append(ratio if j else b"-1")
                want[2].append(gc)
        records = np.concatenate(recs)
        assert len(records) > 520_000
        got, n_lines = T.device_format(tel, records, segs)
        assert n_lines == len(records)
        for k, t in enumerate((T.DENSITY, T.CANON_RATIO, T.GC)):
            vals = [ln.rsplit(b"\t", 1)[1] for ln in got[t].split(b"\n")[:-1]]
            assert vals == want[k], "track %d" % t
    finally:
        tel.close()


def test_value_outside_the_domain_fails_the_call(tel_1000):
    """A density of 200 cannot come from a scan and is not in the formatter's domain: TS_ERR_UNSUPPORTED naming the window, no text."""
    from teloscope_amd import _capi as K
    w, s = 1000, 500
    segs = layout([10 * s], s)
    records = random_records(np.random.default_rng(1), seg_sizes(10 * s, w, s))
    records[5] = [0, 0, 0, 0, 0, 0, 200 * w, 0]
    with pytest.raises(K.TeloscanError) as e:
        T.device_format(tel_1000, records, segs)
    assert e.value.code == K.TS_ERR_UNSUPPORTED and "window 5" in str(e.value)
    records[5] = [2000, 0, 0, 0, 0, 0, 1, 0]                        # a nucleotide count above the window size
    with pytest.raises(K.TeloscanError) as e:
        T.device_format(tel_1000, records, segs)
    assert e.value.code == K.TS_ERR_UNSUPPORTED and "window 5" in str(e.value)
    big = [(0, 10, 0, 10 * s, b"n" * ((1 << 24) + 1))]            # a name the 32-bit line lengths are not made for: refused, by name
    with pytest.raises(K.TeloscanError) as e:
        T.device_format(tel_1000, records, big)
    assert e.value.code == K.TS_ERR_UNSUPPORTED and "16 MiB" in str(e.value)
    check(tel_1000, random_records(np.random.default_rng(2), seg_sizes(10 * s, w, s)), segs, w, s, (1, 1, 1))    # the context still works


def test_wave_starts_at_every_residue_mod_16(tel_1000):
    """Names of 1 to 16 bytes over 17 segments of 65 windows: the 64 lines of a wave start on every residue modulo 16 of their
    file — which the reference text says before the device is asked (a track's block starts 256-byte aligned, so a wave's first
    byte has its line's offset modulo 16) — so the head, body and tail stores of the copy-out (text_store_core.h) meet every
    shift of the staging area."""
    w, s = 1000, 500
    lens = [65 * s] * 17
    segs = layout(lens, s, names=[bytes(97 + (i + k) % 26 for k in range(1 + i % 16)) for i in range(17)])
    assert [sg[1] for sg in segs] == [65] * 17 and {len(sg[4]) for sg in segs} == set(range(1, 17))
    records = random_records(np.random.default_rng(16), [x for ln in lens for x in seg_sizes(ln, w, s)])
    want = T.format_tracks(records, segs, w, s, 1, 1, 1)
    residues = set()
    for text in want:
        lines = text.split(b"\n")[:-1]
        assert len(lines) == 17 * 65
        starts = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])])
        residues |= {int(starts[k]) % 16 for k in range(0, len(lines), 64)}
    assert residues == set(range(16))
    check(tel_1000, records, segs, w, s, (1, 1, 1), want)
