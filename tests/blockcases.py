"""Hand-built match layouts for the block-calling thresholds (host only).

A layout is a background proved match-free for the pattern set plus copies of the set's patterns at chosen positions, so
every case knows its match list exactly.  Each case carries the blocks the reference's rules give for it, written out as
literal data (src/teloscope.cpp:29-256 getTerminalBlocks / getInterstitialBlocks, :543-583 the tips-only scan,
src/read-filter.cpp the read filter).  The oracle must reproduce them (tests/test_oracle_block_thresholds.py) and every
device route must reproduce the oracle (tests/test_gpu_block_thresholds.py).

Motifs: F = CCCTAA (forward list, canonical), R = TTAGGG (reverse list, canonical), FN = CCCTAT and RN = ATAGGG (one
substitution away under -x 1: forward / reverse, non-canonical).  All copies are 6 bases, so a chain gap (difference of
match starts) of g between tandem copies is g, and a sub-block of c tandem copies is 6c long.
"""
import numpy as np

F, R, FN, RN = "CCCTAA", "TTAGGG", "CCCTAT", "ATAGGG"
BG = "A"
LONG20 = "CA" * 10                  # sorts before CCCTAA: the first pattern of a -x 0 set that holds it (minLength 40)
WIDE = "GATCGGTACCATGCAGTCGATCCGTAGCTAGGCATC"     # 36 bases: takes the general kernels' wide form; never occurs here
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def tandem(pos, count, motif=F):
    return [(pos + 6 * i, motif) for i in range(count)]


class Layout:
    """n bases of background with motif copies at [(pos, motif)] (sorted, non-overlapping)."""

    def __init__(self, n, marks):
        self.n = n
        self.marks = sorted(marks)
        for (a, ma), (b, _) in zip(self.marks, self.marks[1:]):
            assert a + len(ma) <= b, "overlapping copies at %d and %d" % (a, b)
        assert not self.marks or self.marks[-1][0] + len(self.marks[-1][1]) <= n

    def seq(self):
        s = bytearray(BG.encode() * self.n)
        for p, m in self.marks:
            s[p:p + len(m)] = m.encode()
        return bytes(s)

    def shifted(self, pad, tail=0):
        """pad bases of background in front, tail at the back"""
        return Layout(self.n + pad + tail, [(p + pad, m) for p, m in self.marks])

    def mirrored(self):
        """the reverse complement: the forward list becomes the reverse list and position p of a 6-mer goes to n - p - 6"""
        return Layout(self.n, [(self.n - p - len(m), revcomp(m)) for p, m in self.marks])

    def with_marks(self, extra, n=None):
        return Layout(self.n if n is None else n, self.marks + list(extra))


class B(tuple):
    """Expected block: (start, block_len, block_counts, forward_count, canonical_count, label, has_valid_or)."""

    def __new__(cls, start, length, counts, fwd, canon, label, valid_or=1):
        return tuple.__new__(cls, (start, length, counts, fwd, canon, label, valid_or))

    def shifted(self, pad):
        return B(self[0] + pad, *self[1:])

    def mirrored(self, n):
        s, ln, c, f, cn, lab, v = self
        return B(n - s - ln, ln, c, c - f, cn, {"p": "q", "q": "p"}.get(lab, lab), v)


class Case:
    """name; cli without -t; t; layout; expected terminal and interstitial blocks; `side` 'p', 'q' or 'its' (which end a
    deciding pair is counted from, or the interstitial walk); `pair` = indices (i, j) into layout.marks of the two matches
    whose gap decides the case (None where no single pair does: zone and n/t edges stay where they are)."""

    def __init__(self, name, cli, t, layout, term, its=(), side="p", pair=None, full=False):
        self.name, self.cli, self.t, self.layout = name, cli, t, layout
        self.term, self.its, self.side, self.pair, self.full = list(term), list(its), side, pair, full

    def command(self, t=None):
        return "x.fa %s -t %d%s" % (self.cli, self.t if t is None else t, " -r -i" if self.full else "")

    def mirrored(self):
        n = self.layout.n
        i, j = self.pair if self.pair else (None, None)
        m = len(self.layout.marks)
        return Case(self.name.replace("p_", "q_", 1), self.cli, self.t, self.layout.mirrored(),
                    sorted((b.mirrored(n) for b in self.term), key=lambda b: -b[0]), [b.mirrored(n) for b in self.its][::-1],
                    {"p": "q", "q": "p"}.get(self.side, self.side), (m - 1 - j, m - 1 - i) if self.pair else None, self.full)

    def deciding_positions(self):
        i, j = self.pair
        return self.layout.marks[i][0], self.layout.marks[j][0]


def _p(name, cli, marks, term, pair, n=5000, t=2000):
    return Case("p_" + name, cli, t, Layout(n, marks), term, side="p", pair=pair)


# Terminal walk, p side (every one is mirrored onto the q side below).  tips-only scans, n = 5000, -t 2000.
P_CASES = [
    # chain gap -k: exactly k chains, k + 1 cuts (-d 5 keeps the two halves apart)
    _p("k_eq", "-k 20 -d 5 -l 60", tandem(100, 10) + tandem(174, 10), [B(100, 134, 20, 20, 20, "p")], (9, 10)),
    _p("k_plus1", "-k 20 -d 5 -l 60", tandem(100, 10) + tandem(175, 10),
       [B(100, 60, 10, 10, 10, "p"), B(175, 60, 10, 10, 10, "p")], (9, 10)),
    # minBlockCounts (2): a one-match sub-block is dropped, a two-match one is kept and merges
    _p("counts_1", "-k 20 -d 40 -l 60", [(100, F)] + tandem(150, 10), [B(150, 60, 10, 10, 10, "p")], (0, 1)),
    _p("counts_2", "-k 20 -d 40 -l 60", tandem(100, 2) + tandem(150, 10), [B(100, 110, 12, 12, 12, "p")], (1, 2)),
    # a sub-block needs a canonical match
    _p("canon_0", "-k 20 -d 40 -l 60 -y 0.4", [(100, FN), (106, FN)] + tandem(150, 10), [B(150, 60, 10, 10, 10, "p")], (1, 2)),
    _p("canon_1", "-k 20 -d 40 -l 60 -y 0.4", [(100, F), (106, FN)] + tandem(150, 10), [B(100, 110, 12, 12, 11, "p")], (1, 2)),
    # density, exact in float32: canCovered 6 >= 0.5 * 12 holds, 6 >= 0.5 * 13 does not
    _p("dens_eq", "-k 20 -d 40 -l 60 -y 0.5", [(100, F), (106, FN)] + tandem(150, 10), [B(100, 110, 12, 12, 11, "p")], (0, 1)),
    _p("dens_below", "-k 20 -d 40 -l 60 -y 0.5", [(100, F), (107, FN)] + tandem(150, 10), [B(150, 60, 10, 10, 10, "p")], (0, 1)),
    # density decided by float32 rounding: float32(0.3) * 100 rounds up to 30.000002 > 30 (rejected, where 0.3 * 100 = 30
    # in decimal would pass); float32(0.3) * 99 = 29.7 < 30 (kept).  test_density_cases_sit_where_float32_puts_them says so.
    _p("dens_f32_len100", "-k 20 -d 5 -l 60 -y 0.3", tandem(100, 5) + [(144, FN), (164, FN), (184, FN), (194, FN)], [], (7, 8)),
    _p("dens_f32_len99", "-k 20 -d 5 -l 60 -y 0.3", tandem(100, 5) + [(144, FN), (164, FN), (184, FN), (193, FN)],
       [B(100, 99, 9, 9, 5, "p")], (7, 8)),
    # merge gap -d (sub-blocks of 60 < -l 100: only the merged block is long enough)
    _p("d_eq", "-k 20 -d 40 -l 100", tandem(100, 10) + tandem(200, 10), [B(100, 160, 20, 20, 20, "p")], (9, 10)),
    _p("d_plus1", "-k 20 -d 40 -l 100", tandem(100, 10) + tandem(201, 10), [], (9, 10)),
    # merged length -l
    _p("l_eq", "-k 20 -d 5 -l 60", tandem(100, 10), [B(100, 60, 10, 10, 10, "p")], (8, 9)),
    _p("l_minus1", "-k 20 -d 5 -l 61", tandem(100, 10), [], (8, 9)),
]
Q_CASES = [c.mirrored() for c in P_CASES]

# inZone and the walk's stop, n = 4000 = 2t (a tips-only scan reads the whole segment): forward zone rel < t, reverse
# zone rel >= n - t; n == t and n == t + 1 put everything in the zone (their difference, rel n - 1 / 0, holds no block)
ZONE = "-k 20 -d 5 -l 60"
ZONE_CASES = [
    Case("zone_fwd_first_at_t-1", ZONE, 2000, Layout(4000, tandem(1999, 10)), [B(1999, 60, 10, 10, 10, "p", 0)], side="p"),
    Case("zone_fwd_first_at_t", ZONE, 2000, Layout(4000, tandem(2000, 10)), [], side="p"),
    Case("zone_rev_first_at_n-t", ZONE, 2000, Layout(4000, tandem(1946, 10, R)), [B(1946, 60, 10, 0, 10, "q", 0)], side="q"),
    Case("zone_rev_first_at_n-t-1", ZONE, 2000, Layout(4000, tandem(1945, 10, R)), [], side="q"),
    Case("zone_n_eq_t", ZONE, 2000, Layout(2000, tandem(1940, 10) + tandem(0, 10, R)),
         [B(1940, 60, 10, 10, 10, "p", 0), B(0, 60, 10, 0, 10, "q", 0)], side="p"),
    Case("zone_n_eq_t+1", ZONE, 2000, Layout(2001, tandem(1940, 10) + tandem(0, 10, R)),
         [B(1940, 60, 10, 10, 10, "p", 0), B(0, 60, 10, 0, 10, "q", 0)], side="p"),
    # the walk ends at the first chain head outside the zone: the block at 2005 is never called
    Case("zone_walk_stops", ZONE, 2000, Layout(4000, tandem(100, 10) + tandem(1900, 10) + tandem(2005, 10)),
         [B(100, 60, 10, 10, 10, "p"), B(1900, 60, 10, 10, 10, "p")], side="p"),
    # hasValidOr at leftDist == rightDist (470 == 1000 - 530) and one base off, both directions
    Case("validor_tie_p", ZONE, 2000, Layout(1000, tandem(470, 10)), [B(470, 60, 10, 10, 10, "p", 1)], side="p"),
    Case("validor_off_p", ZONE, 2000, Layout(1000, tandem(471, 10)), [B(471, 60, 10, 10, 10, "p", 0)], side="p"),
    Case("validor_tie_q", ZONE, 2000, Layout(1000, tandem(470, 10, R)), [B(470, 60, 10, 0, 10, "q", 1)], side="q"),
    Case("validor_off_q", ZONE, 2000, Layout(1000, tandem(469, 10, R)), [B(469, 60, 10, 0, 10, "q", 0)], side="q"),
]
# GFA ends of the valid-orientation cases (walkSegment: a block goes to the start side when distToStart <= distToEnd)
ENDS = {"validor_tie_p": (60, 0), "validor_off_p": (0, 60), "validor_tie_q": (60, 0), "validor_off_q": (60, 0)}


def _i(name, marks, its, pair, cli="-k 20", n=3000, t=100, term=()):
    return Case("its_" + name, cli, t, Layout(n, marks), term, its, side="its", pair=pair, full=True)


# Interstitial walk: full scans, -t 100 keeps the tracks at 1000 out of both zones (boundaries = the segment's ends)
ITS_CASES = [
    _i("canon_4", tandem(1000, 4), [B(1000, 24, 4, 4, 4, "p")], (2, 3)),
    _i("canon_3", tandem(1000, 3) + [(1018, FN)], [], (2, 3)),
    # the 'b' label: 2/2, 1/3 and 3/1 are kept and labelled.  The reference's exclusion of a 'b' block with fewer than two
    # forward AND fewer than two reverse matches (src/teloscope.cpp:216) is dead code: a block needs four canonical matches,
    # so forward + reverse >= 4.  The 1/1, 1/2 and 2/1 cases are empty because of that count, not the label; nothing here
    # (or anywhere) can pin the exclusion itself.
    _i("b_1_1", [(1000, F), (1006, R)], [], (0, 1)),
    _i("b_1_2", [(1000, F), (1006, R), (1012, R)], [], (1, 2)),
    _i("b_2_1", [(1000, F), (1006, F), (1012, R)], [], (1, 2)),
    _i("b_2_2", [(1000, F), (1006, F), (1012, R), (1018, R)], [B(1000, 24, 4, 2, 4, "b")], (2, 3)),
    _i("fr_1_3", [(1000, F), (1006, R), (1012, R), (1018, R)], [B(1000, 24, 4, 1, 4, "q")], (2, 3)),
    _i("fr_3_1", [(1000, F), (1006, F), (1012, F), (1018, R)], [B(1000, 24, 4, 3, 4, "p")], (2, 3)),
    # merge gap -k
    _i("k_eq", tandem(1000, 2) + tandem(1026, 2), [B(1000, 38, 4, 4, 4, "p")], (1, 2)),
    _i("k_plus1", tandem(1000, 2) + tandem(1027, 2), [], (1, 2)),
    # its_evaluate walks a listed chain 64 records per step from the chain's first record: a chain whose -k gap lies
    # between chain records 62/63, 63/64 (across the step) and 64/65, at k and k + 1
    _i("chain_k_eq_at_62", tandem(1000, 63) + tandem(1392, 4), [B(1000, 416, 67, 67, 67, "p")], (62, 63)),
    _i("chain_k_plus1_at_62", tandem(1000, 63) + tandem(1393, 4),
       [B(1000, 378, 63, 63, 63, "p"), B(1393, 24, 4, 4, 4, "p")], (62, 63)),
    _i("chain_k_eq_at_63", tandem(1000, 64) + tandem(1398, 4), [B(1000, 422, 68, 68, 68, "p")], (63, 64)),
    _i("chain_k_plus1_at_63", tandem(1000, 64) + tandem(1399, 4),
       [B(1000, 384, 64, 64, 64, "p"), B(1399, 24, 4, 4, 4, "p")], (63, 64)),
    _i("chain_k_eq_at_64", tandem(1000, 65) + tandem(1404, 4), [B(1000, 428, 69, 69, 69, "p")], (64, 65)),
    _i("chain_k_plus1_at_64", tandem(1000, 65) + tandem(1405, 4),
       [B(1000, 390, 65, 65, 65, "p"), B(1405, 24, 4, 4, 4, "p")], (64, 65)),
    # minLength = 2 * len(patterns.front()): the 20-base first pattern makes it 40
    _i("len_eq_2x_first", tandem(1000, 3) + [(1034, F)], [B(1000, 40, 4, 4, 4, "p")], (2, 3),
       cli="-x 0 -k 30 -p %s,%s,%s" % (LONG20, F, R)),
    _i("len_2x_first_minus1", tandem(1000, 3) + [(1033, F)], [], (2, 3), cli="-x 0 -k 30 -p %s,%s,%s" % (LONG20, F, R)),
    # the fences: the first match at fwdBoundary (160) is walked, the one at revBoundary (2800) is not
    _i("fwd_fence_eq", tandem(100, 10) + tandem(160, 4, R), [B(160, 24, 4, 0, 4, "q")], None,
       cli="-k 20 -d 5 -l 60", t=300, term=[B(100, 60, 10, 10, 10, "p")]),
    _i("fwd_fence_plus1", tandem(100, 10) + tandem(161, 4, R), [B(161, 24, 4, 0, 4, "q")], None,
       cli="-k 20 -d 5 -l 60", t=300, term=[B(100, 60, 10, 10, 10, "p")]),
    _i("rev_fence_eq", tandem(2782, 3) + tandem(2800, 10, R), [], None,
       cli="-k 20 -d 5 -l 60", t=300, term=[B(2800, 60, 10, 0, 10, "q")]),
    _i("rev_fence_4", tandem(2776, 4) + tandem(2800, 10, R), [B(2776, 24, 4, 4, 4, "p")], None,
       cli="-k 20 -d 5 -l 60", t=300, term=[B(2800, 60, 10, 0, 10, "q")]),
    # a terminal block that fails -l leaves fwdBoundary where it was: its matches are walked as an interstitial chain
    _i("l_fail_keeps_fence", tandem(100, 10), [B(100, 60, 10, 10, 10, "p")], None, cli="-k 20 -d 5 -l 61", t=300),
    _i("l_pass_moves_fence", tandem(100, 10), [], None, cli="-k 20 -d 5 -l 60", t=300, term=[B(100, 60, 10, 10, 10, "p")]),
]

# Tips-only scan: n == 2t reads the whole segment, n == 2t + 1 reads [0, t) and [n - t, n) and a copy across t or n - t
# is no match (processRegion bounds scanLimit by the region's end)
TIPS = "-k 20 -d 5 -l 40"
TIPS_CASES = [
    Case("tips_n_2t_fwd", TIPS, 500, Layout(1000, tandem(450, 9)), [B(450, 54, 9, 9, 9, "p")], side="p"),
    Case("tips_n_2t+1_fwd", TIPS, 500, Layout(1001, tandem(450, 9)), [B(450, 48, 8, 8, 8, "p")], side="p"),
    Case("tips_n_2t_rev", TIPS, 500, Layout(1000, tandem(495, 10, R)), [B(495, 60, 10, 0, 10, "q")], side="q"),
    Case("tips_n_2t+1_rev", TIPS, 500, Layout(1001, tandem(495, 10, R)), [B(501, 54, 9, 0, 9, "q")], side="q"),
]

TERMINAL_CASES = P_CASES + Q_CASES + ZONE_CASES + TIPS_CASES
ALL_CASES = TERMINAL_CASES + ITS_CASES


def scanned_regions(case):
    """where a scan of this case reads matches from (the tips-only split of src/teloscope.cpp:576-583)"""
    n, t = case.layout.n, case.t
    if case.full or n <= 2 * t:
        return [(0, n)]
    return [(0, t), (n - t, n)]


def expected_matches(case):
    """(position, size, forward, canonical) of every copy inside a scanned region"""
    fwd = {F: (1, 1), FN: (1, 0), R: (0, 1), RN: (0, 0)}
    out = []
    for p, m in case.layout.marks:
        if any(a <= p and p + len(m) <= b for a, b in scanned_regions(case)):
            out.append((p, len(m)) + fwd[m])
    return out


# Read filter (--fastq-subset: -l 42 unless given, the whole read is terminal zone).  (name, cli, marks, passes); reads
# are 300 bases with the track at their start, and each is also checked reverse-complemented (the reverse list).
READ_CASES = [
    ("l_eq", "", tandem(0, 5) + [(36, F)], True),
    ("l_minus1", "", tandem(0, 5) + [(35, F)], False),
    ("k_eq", "-k 20 -d 5 -l 60", tandem(0, 5) + tandem(44, 5), True),
    ("k_plus1", "-k 20 -d 5 -l 60", tandem(0, 5) + tandem(45, 5), False),
    ("d_eq", "-k 20 -d 40 -l 100", tandem(0, 10) + tandem(100, 10), True),
    ("d_plus1", "-k 20 -d 40 -l 100", tandem(0, 10) + tandem(101, 10), False),
    ("y_f32_len100", "-k 20 -d 5 -l 60 -y 0.3", tandem(0, 5) + [(44, FN), (64, FN), (84, FN), (94, FN)], False),
    ("y_f32_len99", "-k 20 -d 5 -l 60 -y 0.3", tandem(0, 5) + [(44, FN), (64, FN), (84, FN), (93, FN)], True),
    ("y_eq", "-l 12 -y 0.5", [(0, F), (6, FN)], True),
    ("y_below", "-l 12 -y 0.5", [(0, F), (7, FN)], False),
]
# the pair of each read case whose gap decides it (indices into its sorted marks)
READ_PAIRS = {"l_eq": (4, 5), "l_minus1": (4, 5), "k_eq": (4, 5), "k_plus1": (4, 5), "d_eq": (9, 10), "d_plus1": (9, 10),
              "y_f32_len100": (7, 8), "y_f32_len99": (7, 8), "y_eq": (0, 1), "y_below": (0, 1)}
READ_LEN = 300


def read_layout(marks, n=READ_LEN):
    return Layout(n, marks)


def filler_spacing(cli, full=False):
    """single copies this far apart never chain (gap > -k): each is a one-match sub-block (dropped before -d is applied)
    or a one-match interstitial chain (fewer than four canonical matches), so they add no block and merge with nothing.
    A full scan misses a copy across a window's end (the window scan stops its walk there, src/teloscope.cpp:439): there
    the spacing also divides the window and the step, so no filler lies across one."""
    import teloscope_amd.cli as tc
    o = tc.parse_cli("x.fa " + cli)
    lo = max(o.max_match_dist + 1, 6)
    if not full:
        return lo + 6
    d = next(d for d in range(lo, o.step + 1) if o.step % d == 0 and o.window_size % d == 0)
    return d


def at_record_index(layout, pair, index, side, spacing, motif=None):
    """The layout with single filler copies added so that the pair's second record in walk order is record `index` of the
    record stream that holds the layout (every record, either list): counted from the start for side 'p' / 'its' (copies
    in front) and from the end for side 'q' (copies behind).  Whether that stream lies in one tile of a plan is for the
    caller to assert.  Returns (layout, shift of the original positions), or None when the pair already lies deeper."""
    i, j = pair
    m = len(layout.marks)
    if side == "q":
        need = index - (m - 1 - i)                   # (walked from the end: the pair's second record is its lower one)
        if need < 0:
            return None
        end = layout.n
        extra = [(end + spacing * (c + 1) - 6, motif or R) for c in range(need)]
        return Layout(end + spacing * need, layout.marks + extra), 0
    need = index - j
    if need < 0:
        return None
    pad = spacing * need
    lay = layout.shifted(pad)
    extra = [(spacing * c, motif or F) for c in range(need)]
    return Layout(lay.n, lay.marks + extra), pad


def f32_density_side(can_covered, length, density):
    """True when canCovered >= minBlockDensity * (blockEnd - blockStart) holds in float32, as the reference evaluates it"""
    return bool(np.float32(can_covered) >= np.float32(np.float32(density) * np.float32(length)))


LONG_READ_RECORDS = 140                  # above the predicate's long-list threshold of 128 records


def long_read(lay, pair, index, cli, motif):
    """A read whose deciding pair is record `index` of its record stream counted from the start (pred_scan_wave walks
    both lists in ascending order), topped up behind the track with single copies to LONG_READ_RECORDS records.
    Returns (layout, shift of the original positions)."""
    spacing = filler_spacing(cli)
    lr, shift = at_record_index(lay, pair, index, "p", spacing, motif)
    top = LONG_READ_RECORDS - len(lr.marks)
    return lr.with_marks([(lr.n + spacing * (c + 1) - 6, motif) for c in range(top)], n=lr.n + spacing * top), shift
