"""Hand-built segments for the general kernels' tile, halo, window and list-capacity edges (host only; no tests here).

The general kernels (teloscope_amd/csrc/generic.hip) cut a scanned region into tiles of B = TS_GENERAL_TILE positions from
the region's start and stage HALO bases beyond each (kHalo = 32 for the list and the position-strided form, TS_WIDE_HALO for
the wide form).  Every case here is (command line, segments, what each segment is for): a background of random C and G —
no pattern of any set used here is free of A and T, so the background holds no match — plus copies of the set's repeat unit
at chosen positions.  Each segment lists the intervals it planted; tests/test_general_tile_cases_cpu.py proves from the
oracle and from a plain Python search that every match lies in one, and that each case is what it claims to be;
tests/test_gpu_general_tiles.py runs every case through every form it names.

What the cases pin, and where the edge was read (generic.hip unless said otherwise):
  straddle       matches starting at every position of [iB - L, iB + 1]: halo reads (:336, :606, wide :884), the wave ranges of
                 the candidate lists (:655) and the per-tile record slots (:414, :844)
  halo end       a longest pattern starting at B - 1 reads the last halo base; avail clamps (pipeline.cpp:1210, :343, :666)
  lengths        segments of B - 1 .. 2B + 1 bases with a match ending on the last base (T.n / T.avail of the last tile)
  invalid        a non-ACGT byte at B - 1, B and B + HALO - 1 (:344, the slow path :663-685, stage16 :462)
  homopolymer    whole tiles of one base: the packed nucleotide counters (:40-43 8-bit fields, :491 / :507 16-bit halves) and a
                 wave's list exactly full with one candidate per position (:689)
  windows        record spans against tiles: record_in_tile (:152), the list form's own test (:827), kw_lo / rec_hi (:710-715),
                 div_step (:519) at s = 8192 / 8193, the list-form edge of pipeline.cpp:1258 against kWaccMax (:429, :715)
  capacity       1023, 1024 and 1025 candidates in one wave's list (kListWave, :430, :689)
  tips           a second region that starts on and off a 16-byte offset (:300, :612; pipeline.cpp:1192, :1216)
"""
import ctypes as C
import os
import re
import zlib

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "teloscope_amd", "csrc")


def _constant(path, pattern):
    return int(re.search(pattern, open(os.path.join(_CSRC, path)).read()).group(1))


B = _constant("ts_internal.h", r"#define TS_GENERAL_TILE (\d+)")
WIDE_HALO = _constant("ts_internal.h", r"#define TS_WIDE_HALO (\d+)")
HALO = _constant("generic.hip", r"constexpr uint32_t kHalo = (\d+);")
LIST_WAVE = _constant("generic.hip", r"constexpr uint32_t kListWave = (\d+);")


def list_max_records():
    """ts_k_general_list_max_records() of the built library: the window records a tile may add to in the list form"""
    from teloscope_amd import _capi as K
    f = getattr(K.lib(), "_Z29ts_k_general_list_max_recordsv")
    f.restype, f.argtypes = C.c_uint32, []
    return int(f())


LIST_MAX_RECORDS = list_max_records()

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return bytes(b).translate(_COMP)[::-1]


def background(name, n):
    """n bases of seeded random C / G"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return bytearray(np.frombuffer(b"CG", dtype=np.uint8)[rng.integers(0, 2, size=n)].tobytes())


def array_text(unit, length, phase):
    """`length` bases of the unit's perfect array; a unit starts at every offset = phase (mod len(unit))"""
    u = len(unit)
    return bytes(unit[(p - phase) % u] for p in range(length))


class Seg:
    """one segment: its bases, what it is for, the [a, b) intervals that were planted, and the facts the CPU test checks"""

    def __init__(self, name, n):
        self.name, self.n = name, n
        self.buf = background(name, n)
        self.planted = []
        self.what = name
        self.facts = {}

    def plant(self, at, text):
        """text at position `at`, cut to the segment"""
        a, b = max(0, at), min(self.n, at + len(text))
        if a < b:
            self.buf[a:b] = text[a - at:b - at]
            self.planted.append((a, b))
        return self

    def plant_array(self, a, b, unit, phase, rc=False):
        """the unit's array over [a, b): forward, a unit starts at every position = phase (mod len(unit)); rc, the reverse
        complement of such a text (the reverse patterns match it)"""
        a, b = max(0, a), min(self.n, b)
        if a < b:
            if rc:
                t = revcomp(array_text(unit, b - a, (b - phase) % len(unit)))     # position-anchored as well: overlapping plants agree
            else:
                t = array_text(unit, b - a, (phase - a) % len(unit))
            self.plant(a, t)
        return self

    @property
    def seq(self):
        return bytes(self.buf)


class PatternSet:
    def __init__(self, name, cli, unit, lengths, longest, forms, wide=False, halo=None, forced=False):
        self.name, self.cli, self.unit, self.lengths, self.longest = name, cli, unit, tuple(lengths), longest
        self.forms, self.wide, self.forced = forms, wide, forced
        self.halo = halo if halo is not None else (WIDE_HALO if wide else HALO)
        self.lmax = max(lengths)


U6 = b"TTAGGG"
K32 = (U6 * 6)[:32]                     # the 32-base unit of GENERIC_GRID (tests/test_gpu_parity.py): the longest the table forms take
K63 = (U6 * 11)[:63]                    # WIDE_GRID's 63-base pattern: the longest a ts_pattern holds
U11 = b"TTA" + b"A" * 8                 # the unit whose array holds every pattern of WIDE_GRID's nine-length set (TTA, TTAA, ... 3..11)
NINE = [b"TTA" + b"A" * i for i in range(9)]

NO_ENV = ()
STRIDED = (("TS_GEN_LIST", "0"),)
FORCED = (("TS_FORCE_GENERAL", "1"),)
BOTH = [NO_ENV, STRIDED]

LIST_SET = PatternSet("mixed56", "-p TTAGGG,TTAGG -x 0", U6, (5, 6), U6, BOTH)
K32_SET = PatternSet("k32", "-c %s -x 0" % K32.decode(), U6, (32,), K32, BOTH)
MIX32_SET = PatternSet("mixed6_32", "-p TTAGGG,%s -x 0" % K32.decode(), U6, (6, 32), K32, BOTH)
WIDE63_SET = PatternSet("wide6_63", "-c TTAGGG -p TTAGGG,%s -x 0" % K63.decode(), U6, (6, 63), K63, [NO_ENV], wide=True)
WIDE9_SET = PatternSet("wide_nine", "-x 0 -p " + ",".join(p.decode() for p in NINE), U11, range(3, 12), NINE[-1], [NO_ENV], wide=True)
K6_SET = PatternSet("forced_k6", "-c TTAGGG -x 0", U6, (6,), U6, [FORCED, FORCED + STRIDED], forced=True)
POLY_SET = PatternSet("forced_polyA", "-c AAAAAA -x 0", b"A", (6,), b"AAAAAA", [FORCED, FORCED + STRIDED], forced=True)
CAP_SET = PatternSet("polyA56", "-p AAAAAA,AAAAA -x 0", b"A", (5, 6), b"AAAAAA", [NO_ENV])
ALL_SETS = [LIST_SET, K32_SET, MIX32_SET, WIDE63_SET, WIDE9_SET, K6_SET]

TIPS = ""                                        # the reference's default: a tips-only scan, -t 50000 (one region up to 100 kb)
FULL = "-w 1000 -s 500 -r -g -e -m -i"           # every match is pushed: the patterns are shorter than step and overlap


class Case:
    """name; family; pattern set; cli; segments; forms = the environments it runs under; fold = the context's case folding;
    tiled_twin = the default route of this command is the tiled kernel, whose output the forced general run must equal"""

    def __init__(self, name, family, pset, scan, segs, forms=None, fold=True, spills=False):
        self.name, self.family, self.pset, self.segs, self.fold, self.spills = name, family, pset, segs, fold, spills
        self.cli = "x.fa %s %s" % (pset.cli, scan)
        self.forms = list(pset.forms if forms is None else forms)
        self.tiled_twin = False

    def __repr__(self):
        return self.name

    def options(self):
        from teloscope_amd.cli import parse_cli
        return parse_cli(self.cli)

    def expected_form(self, env):
        """'wide', 'list' or 'strided': the form the fused pass must END in under `env` — the host's rule (pipeline.cpp:1258,
        capi_internal.hpp ts_general_list_form_ok) and the one case whose wave list spills (generic.hip:689)"""
        o = self.options()
        if self.pset.wide:
            return "wide"
        if ("TS_GEN_LIST", "0") in env or self.spills or o.step < 2 or o.window_size >= (1 << 28):
            return "strided"
        if o.ultra_fast:
            return "list"
        return "list" if (B + o.window_size) // o.step + 3 <= LIST_MAX_RECORDS else "strided"


def _phases(pset):
    return range(len(pset.unit))


def _tag(scan):
    return "tips" if scan == TIPS else "full"


# ------------------------------------------------------------------------------------------------------------ placements
def straddle_case(pset, scan):
    """the unit's array across the tile boundaries B and 2B, forward and reverse complement, at every phase: over the
    case's segments a match of every length starts at every position of [iB - L, iB + 1]"""
    n, u, L = 3 * B + 12, len(pset.unit), pset.lmax
    segs = []
    for rc in (False, True):
        for ph in _phases(pset):
            s = Seg("straddle %s %s rc=%d phase=%d" % (pset.name, _tag(scan), rc, ph), n)
            for i in (1, 2):
                s.plant_array(i * B - 2 * L - 2 * u, i * B + 2 + 2 * L + 2 * u, pset.unit, ph, rc)
            s.facts = dict(boundaries=(B, 2 * B), rc=rc)
            segs.append(s)
    return Case("straddle-%s-%s" % (pset.name, _tag(scan)), "straddle", pset, scan, segs)


def halo_end_case(pset, scan):
    """one occurrence of the longest pattern (length L) starting at B - 1 (it reads halo bases 0 .. L - 2: the last one when
    L = HALO + 1, the wide form's 63 of 64 one short of it), at B - L and at B - L + 1, in segments of B - 1 + L bases (the
    match at B - 1 ends on the last base), one base fewer (it does not fit: no match), B + HALO and B + HALO + 1"""
    L, halo = pset.lmax, pset.halo
    segs = []
    for rc in (False, True):
        text = revcomp(pset.longest) if rc else pset.longest
        for start in (B - 1, B - L, B - L + 1):
            for n in (B - 1 + L, B - 2 + L, B + halo, B + halo + 1):
                s = Seg("halo end %s %s rc=%d start=%d n=%d" % (pset.name, _tag(scan), rc, start, n), n)
                s.plant(start, text)
                s.facts = dict(start=start, L=L, whole=start + L <= n)
                segs.append(s)
    return Case("halo-end-%s-%s" % (pset.name, _tag(scan)), "halo_end", pset, scan, segs)


SEGMENT_LENGTHS = (B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1)


def lengths_case(pset, scan):
    """segments of B - 1 .. 2B + 1 bases with an array at the very end, the longest pattern ending on the last base"""
    u, L = len(pset.unit), pset.lmax
    segs = []
    for rc in (False, True):
        for n in SEGMENT_LENGTHS:
            s = Seg("length %s %s rc=%d n=%d" % (pset.name, _tag(scan), rc, n), n)
            a = n - L - 3 * u
            # forward: a unit starts at n - L; reverse: the text mirrors one whose unit starts at its first base (n - L again)
            s.plant_array(a, n, pset.unit, (n - L) % u if not rc else n % u, rc)
            s.facts = dict(flush=(n - L, L))
            segs.append(s)
    return Case("lengths-%s-%s" % (pset.name, _tag(scan)), "lengths", pset, scan, segs)


def invalid_case(pset, scan, fold):
    """a non-ACGT byte at B - 1, at B and at B + HALO - 1 inside an array, at every phase: N, an IUPAC code and a lower-case
    letter under a folding context (the letter is then a base: nothing dies), N and a lower-case letter under a strict one"""
    u, L, halo = len(pset.unit), pset.lmax, pset.halo
    n = B + halo + 2 * L + 4 * u + 37
    kinds = ("N", "R", "lower") if fold else ("N", "lower")
    segs = []
    for x in (B - 1, B, B + halo - 1):
        for kind in kinds:
            for ph in _phases(pset):
                s = Seg("invalid %s %s fold=%d at=%d %s phase=%d" % (pset.name, _tag(scan), fold, x, kind, ph), n)
                s.plant_array(B - 1 - 2 * L - 2 * u, B + halo + 2 * L + 2 * u, pset.unit, ph)
                clean = s.seq
                s.buf[x] = s.buf[x] | 0x20 if kind == "lower" else ord(kind)
                s.facts = dict(at=x, kills=not (kind == "lower" and fold), clean=clean)
                segs.append(s)
    return Case("invalid-%s-%s-%s" % (pset.name, _tag(scan), "fold" if fold else "strict"), "invalid", pset, scan, segs, fold=fold)


def homopolymer_case(w, s):
    """whole tiles of A, C, G and T (the second tile of a three-tile segment, and the first of a two-tile one) under the
    forced single-length set AAAAAA: every position of an A or T tile is a candidate (a wave's list is exactly full), and a
    tile's nucleotide counters hold 4096 of one base.  w = s = B: a record is a tile; w = 2B, s = B: main and carry calls
    feed one record"""
    segs = []
    for base in b"ACGT":
        ch = bytes([base])
        a = Seg("homopolymer %d/%d %s second tile" % (w, s, ch.decode()), 3 * B)
        a.plant(B, ch * B)
        b = Seg("homopolymer %d/%d %s first tile" % (w, s, ch.decode()), 2 * B)
        b.plant(0, ch * B)
        for x in (a, b):
            x.facts = dict(base=ch)
        segs += [a, b]
    return Case("homopolymer-%d-%d" % (w, s), "homopolymer", POLY_SET, "-w %d -s %d -r -g -e -m -i" % (w, s), segs)


# --------------------------------------------------------------------------------------------------------- window geometries
def list_edge_geometry(step=32):
    """the largest window at this step whose tiles add to at most ts_k_general_list_max_records() records by the host's rule
    (pipeline.cpp:1258: (B + w) / s + 3 <= max), and the next one"""
    w = (LIST_MAX_RECORDS - 3 + 1) * step - B - 1
    assert (B + w) // step + 3 == LIST_MAX_RECORDS and (B + w + 1) // step + 3 == LIST_MAX_RECORDS + 1
    return (w, step), (w + 1, step)


LIST_EDGE, PAST_LIST_EDGE = list_edge_geometry()
# the smallest step the list form can run at (w = s): below it a tile adds to more records than the form holds, so the multiply
# of div_step (generic.hip:519) never sees s = 2 in this form — only the position-strided form, which divides, does
SMALLEST_LIST_STEP = min(s for s in range(2, B) if (B + s) // s + 3 <= LIST_MAX_RECORDS)
# (w, s): what must hold of the record spans [R s, min(R s + w, n)) against the tiles — asserted by the CPU test
GEOMETRIES = [
    ((B, B), dict(starts=True, ends=True)),
    ((B // 2, B // 4), dict(starts=True, ends=True)),
    ((2 * B, B), dict(starts=True, ends=True, tiles=2)),
    ((B, B // 2), dict(starts=True, ends=True)),
    ((10000, 5000), dict(tiles=3)),                            # a record over three tiles and more
    ((1000, 300), dict(not_multiple=True)),
    ((8, 2), dict(starts=True, ends=True)),
    ((8, 1), dict(starts=True, ends=True)),                    # s = 1: the list form's division needs s >= 2
    ((4 * B, 2 * B), dict(starts=True, ends=True, tiles=4)),   # s = 8192: the last step divided by the multiply
    ((4 * B + 2, 2 * B + 1), dict(tiles=4)),                   # s = 8193: the first divided by the compare
    (LIST_EDGE, dict(tiles=1)),
    (PAST_LIST_EDGE, dict(tiles=1)),
    ((SMALLEST_LIST_STEP, SMALLEST_LIST_STEP), dict(tiles=1)),
]


def window_case(pset, w, s, facts):
    n = (40000 if w >= 4 * B else 2 * B if s <= 2 else 3 * B) + 12
    u, L = len(pset.unit), pset.lmax
    segs = []
    for rc, ph in ((False, 1), (True, 3)):
        sg = Seg("windows %s %d/%d rc=%d" % (pset.name, w, s, rc), n)
        marks = [i * B for i in range(1, n // B + 1)]                                  # tile boundaries
        marks += [k * s for k in range(1, 4)] + [k * s + w for k in range(0, 3)]      # record starts and ends
        rng = np.random.default_rng(zlib.crc32(sg.name.encode()) ^ 5)
        marks += [int(x) for x in rng.integers(0, n, size=12)]
        for m in marks:
            sg.plant_array(m - L - 2 * u, m + L + 2 * u, pset.unit, ph, rc)
        sg.plant_array(n - 3 * u, n, pset.unit, ph, rc)                                # and the segment's end
        sg.facts = dict(w=w, s=s, **facts)
        segs.append(sg)
    return Case("windows-%s-%d-%d" % (pset.name, w, s), "windows", pset, "-w %d -s %d -r -g -e -m -i" % (w, s), segs)


# -------------------------------------------------------------------------------------------------------------- list capacity
def _cap_candidates(runs):
    """a run of R A's under {AAAAAA, AAAAA} lists R - 5 six-mers and R - 4 five-mers: 2 R - 9 candidates, all matches"""
    return sum(2 * r - 9 for r in runs)


def capacity_case(runs):
    """poly-A runs wholly inside positions [1024, 2048) of the second tile — one wave's range (generic.hip:655) — far from
    any window end (w = s = B: a window is a tile), so every candidate is pushed"""
    cand = _cap_candidates(runs)
    s = Seg("capacity %d candidates" % cand, 2 * B + 77)
    at = B + 1024 + 100
    for r in runs:
        s.plant(at, b"A" * r)
        at += r + 40
    assert at < B + 2048 - 50
    s.facts = dict(candidates=cand, lo=B + 1024, hi=B + 2048)
    return Case("capacity-%d" % cand, "capacity", CAP_SET, "-w %d -s %d -r -g -e -m -i" % (B, B), [s], spills=cand > LIST_WAVE)


CAPACITY_RUNS = [(516,), (260, 261), (517,)]              # 1023, 1024 and 1025 candidates


# ------------------------------------------------------------------------------------------------------------------- tips only
TIPS_T = 400


def tips_case():
    """-t 400 with n = 2t (one region), 2t + 1, 2t + 15, 2t + 16 and B + 2t (two regions: the second starts at n - t, on and
    off a 16-byte offset of the segment); an array on each tip and one across each inner region end (no match may cross it)"""
    t, u = TIPS_T, len(U6)
    segs = []
    for rc in (False, True):
        for n in (2 * t, 2 * t + 1, 2 * t + 15, 2 * t + 16, B + 2 * t):
            s = Seg("tips n=%d rc=%d" % (n, rc), n)
            s.plant_array(0, 10 * u, U6, 0, rc)
            s.plant_array(n - 10 * u, n, U6, n % u, rc)
            s.plant_array(t - 3 * u, t + 3 * u, U6, 1, rc)
            s.plant_array(n - t - 3 * u, n - t + 3 * u, U6, 2, rc)
            s.facts = dict(t=t)
            segs.append(s)
    return Case("tips-mixed56-t%d" % t, "tips", LIST_SET, "-t %d" % t, segs)


def _tiled_default(case):
    """does the default route of this command (no TS_FORCE_GENERAL) plan the tiled kernel?  (a planning-only context)"""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import user_input
    return ta.Teloscope(user_input(case.options(), device=K.DEVICE_NONE)).usesFastPath()


def build_cases():
    cases = []
    for pset in ALL_SETS:
        for scan in (TIPS, FULL):
            cases += [straddle_case(pset, scan), halo_end_case(pset, scan), lengths_case(pset, scan),
                      invalid_case(pset, scan, True), invalid_case(pset, scan, False)]
    cases += [homopolymer_case(B, B), homopolymer_case(2 * B, B)]
    for (w, s), facts in GEOMETRIES:
        cases += [window_case(LIST_SET, w, s, facts), window_case(K6_SET, w, s, facts)]
    # the wide form keeps window records of its own (its record_in_tile call, generic.hip:1208): the geometries whose records
    # start and end on tile boundaries, span three tiles, or are no multiple of the step
    for (w, s), facts in GEOMETRIES[:6]:
        cases.append(window_case(WIDE63_SET, w, s, facts))
    cases += [capacity_case(r) for r in CAPACITY_RUNS]
    cases.append(tips_case())
    for c in cases:
        c.tiled_twin = c.pset.forced and _tiled_default(c)
    return cases


CASES = build_cases()
CASE_COUNT = 98                          # asserted by the CPU test against len(CASES) and against the GPU test's parametrization
