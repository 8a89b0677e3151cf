"""The cases of tests/gentilecases.py are what they claim to be — proved on the host, from the oracle and from a plain Python
search that shares no code with it.  A case that fails a condition here is a broken case: none is skipped or filtered."""
import numpy as np
import pytest

from tests import gentilecases as G
from tests.backends import OracleBackend

B = G.B
_ORACLES = {}
_SCANS = {}


def _oracle(case):
    if case.cli not in _ORACLES:
        _ORACLES[case.cli] = OracleBackend(case.options())
    return _ORACLES[case.cli]


def _scan(case, seq):
    """the oracle's segment for these bases as the case's context reads them (a folding context: upper-cased first)"""
    key = (case.cli, case.fold, seq)
    if key not in _SCANS:
        _SCANS[key] = _oracle(case).scan_segment(seq.upper() if case.fold else seq, 0, case.options().ultra_fast)
    return _SCANS[key]


def _matches(case, seq):
    """the oracle's matches: the forward and the reverse list (a tips-only scan fills no other)"""
    r = _scan(case, seq)
    m = np.concatenate([r["fwd_matches"], r["rev_matches"]])
    assert case.options().ultra_fast or len(m) == len(r["all_matches"])
    return [(int(p), int(l), bool(f), bool(c)) for p, l, f, c in zip(m["position"], m["match_size"], m["is_forward"], m["is_canonical"])]


def _merged(intervals):
    """the union of [a, b) intervals (arrays planted side by side or over each other are one array: their phase is by position)"""
    out = []
    for a, b in sorted(intervals):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def _starts(case, seq):
    return {(p, l) for p, l, _, _ in _matches(case, seq)}


# ---------------------------------------------------------------------------------------------------- the second source
def python_matches(case, seq):
    """{(position, length): (forward, canonical)} by bytes.find over every pattern of the -x 0 set and its reverse complement.
    forward: as the harness hands it to the product (teloscope_amd.cli.user_input: the library's own pattern expansion, which
    shares no code with the oracle's); canonical: the pattern is one of the two canonical repeats.  What a scan
    keeps of them: a tips-only scan the matches inside one of its regions ([0, n) up to 2t bases, else [0, t) and [n - t, n));
    a full scan with w == s those inside one window, and with overlapping windows — the patterns here are no longer than the
    overlap — every one (each lies whole in the window whose own part holds its last base)."""
    o = case.options()
    assert o.edit_distance == 0
    if case.fold:
        seq = seq.upper()
    n = len(seq)
    pats = set()
    for p in o.raw_patterns:
        pats |= {p.encode(), G.revcomp(p.encode())}
    if o.ultra_fast:
        t = o.terminal_limit
        regions = [(0, n)] if n <= 2 * t else [(0, t), (n - t, n)]
    elif o.window_size == o.step:
        regions = [(a, min(n, a + o.step)) for a in range(0, n, o.step)]
    else:
        assert max(map(len, pats)) <= o.window_size - o.step or o.step <= 2      # (8/2 and 8/1: worked out in the builder's notes)
        regions = [(0, n)]
    out = {}
    canon = (o.canonical_fwd.encode(), o.canonical_rev.encode())
    from teloscope_amd.cli import user_input
    forward = {p.encode(): f for p, f in user_input(o).patternInfo}
    assert set(forward) == pats
    for p in pats:
        at = seq.find(p)
        while at >= 0:
            if any(a <= at and at + len(p) <= b for a, b in regions):
                out[(at, len(p))] = (forward[p], p in canon)
            at = seq.find(p, at + 1)
    return out


# --------------------------------------------------------------------------------------------------------- whole-list facts
def test_the_case_list_is_complete_and_counted():
    names = [c.name for c in G.CASES]
    assert len(names) == len(set(names)) == G.CASE_COUNT
    from tests import test_gpu_general_tiles as T                          # (imports nothing of the device)
    assert T.CASES is G.CASES
    marks = [m for m in T.test_case_matches_the_oracle_in_every_form.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and len(marks[0].args[1]) == G.CASE_COUNT
    families = {c.family for c in G.CASES}
    assert families == {"straddle", "halo_end", "lengths", "invalid", "homopolymer", "windows", "capacity", "tips"}
    # every placement under every set, table forms and wide, tips-only and full
    for fam in ("straddle", "halo_end", "lengths", "invalid"):
        for pset in G.ALL_SETS:
            for scan in ("tips", "full"):
                assert any(c.family == fam and c.pset is pset and c.name.split("-")[-1 if fam != "invalid" else -2] == scan for c in G.CASES), (fam, pset.name, scan)


def test_segments_stay_small():
    for c in G.CASES:
        o = c.options()
        limit = 40012 if (not o.ultra_fast and o.window_size >= 16384) else 3 * B + 12
        for s in c.segs:
            assert s.n == len(s.seq) <= limit, s.name


def test_pattern_sets_are_what_they_say():
    for pset in G.ALL_SETS + [G.POLY_SET, G.CAP_SET]:
        case = next(c for c in G.CASES if c.pset is pset)
        lens = sorted({len(p[0]) for p in _oracle(case).patterns})
        assert lens == sorted(pset.lengths), pset.name
        assert len(pset.longest) == pset.lmax and pset.halo == (G.WIDE_HALO if pset.wide else G.HALO)
        assert pset.wide == (len(lens) > 8 or pset.lmax > 32), pset.name       # what the table forms cannot hold goes to the wide form


def test_forms_the_cases_must_end_in():
    """the host's rule (pipeline.cpp:1258) on the geometries that sit on its edges, and the one spill"""
    by = {c.name: c for c in G.CASES}
    (we, se), (wp, sp) = G.LIST_EDGE, G.PAST_LIST_EDGE
    assert (B + we) // se + 3 == G.LIST_MAX_RECORDS and (B + wp) // sp + 3 == G.LIST_MAX_RECORDS + 1 and wp == we + 1
    assert by["windows-mixed56-%d-%d" % (we, se)].expected_form(G.NO_ENV) == "list"
    assert by["windows-mixed56-%d-%d" % (wp, sp)].expected_form(G.NO_ENV) == "strided"
    assert by["windows-mixed56-8-1"].expected_form(G.NO_ENV) == "strided"
    assert by["windows-mixed56-8-2"].expected_form(G.NO_ENV) == "strided"       # (s = 2 never reaches the list form's multiply)
    k = G.SMALLEST_LIST_STEP
    assert by["windows-mixed56-%d-%d" % (k, k)].expected_form(G.NO_ENV) == "list" and (B + k - 1) // (k - 1) + 3 > G.LIST_MAX_RECORDS
    assert by["windows-forced_k6-8-1"].expected_form(G.FORCED) == "strided"
    assert [by["capacity-%d" % k].expected_form(G.NO_ENV) for k in (1023, 1024, 1025)] == ["list", "list", "strided"]
    assert G.LIST_WAVE == 1024
    for c in G.CASES:
        for env in c.forms:
            if ("TS_GEN_LIST", "0") in env:
                assert c.expected_form(env) in ("strided", "wide")
    # the forced single-length geometries the tiled kernel takes by default have a twin to be compared with
    for w, s in ((B, B), (B // 2, B // 4), (2 * B, B), (B, B // 2), (10000, 5000), (1000, 300)):
        assert by["windows-forced_k6-%d-%d" % (w, s)].tiled_twin, (w, s)
    assert all(c.tiled_twin for c in G.CASES if c.pset.forced and c.family in ("straddle", "halo_end", "lengths", "invalid", "homopolymer"))


# ------------------------------------------------------------------------------------------------------------ per family
def _straddle(case):
    for rc in (False, True):
        got = set()
        for s in case.segs:
            if s.facts["rc"] == rc:
                got |= _starts(case, s.seq)
        for bound in (B, 2 * B):
            assert bound in case.segs[0].facts["boundaries"]
            for L in case.pset.lengths:
                missing = [p for p in range(bound - L, bound + 2) if (p, L) not in got]
                assert not missing, "%s rc=%d: no match of length %d starts at %s" % (case.name, rc, L, missing)


def _halo_end(case):
    L = case.pset.lmax
    seen = set()
    for s in case.segs:
        f = s.facts
        got = _starts(case, s.seq)
        assert ((f["start"], L) in got) == f["whole"], s.name
        if f["start"] == B - 1 and s.n == B - 1 + L:
            assert f["whole"] and f["start"] == s.n - L and (s.n - L, L) in got, s.name      # ends on the last base: uses halo base L - 2
            seen.add("flush")
        if f["start"] == B - 1 and s.n == B - 2 + L:
            assert not f["whole"] and not any(l == L for _, l in got), s.name                  # one base shorter: none
            seen.add("short")
    assert seen == {"flush", "short"}
    assert {s.n for s in case.segs} == {B - 1 + L, B - 2 + L, B + case.pset.halo, B + case.pset.halo + 1}


def _lengths(case):
    assert sorted({s.n for s in case.segs}) == list(G.SEGMENT_LENGTHS)
    for s in case.segs:
        assert s.facts["flush"] == (s.n - case.pset.lmax, case.pset.lmax) and s.facts["flush"] in _starts(case, s.seq), s.name


def _invalid(case):
    killed_from, killed_to, left, right = set(), set(), set(), set()
    for s in case.segs:
        x, kills = s.facts["at"], s.facts["kills"]
        assert s.seq != s.facts["clean"] and len(s.seq) == len(s.facts["clean"])
        clean = _starts(case, s.facts["clean"])
        touching = {(p, l) for p, l in clean if p <= x < p + l}
        got = _starts(case, s.seq)
        assert got == (clean - touching if kills else clean), s.name
        if kills:
            killed_from |= {x for p, l in touching if p == x}
            killed_to |= {x for p, l in touching if p + l - 1 == x}
            left |= {x for p, l in got if p + l == x}
            right |= {x for p, l in got if p == x + 1}
    edges = {B - 1, B, B + case.pset.halo - 1}
    assert {s.facts["at"] for s in case.segs} == edges
    # at each edge some phase loses a match that starts on the byte and one that ends on it, and keeps both neighbours
    assert killed_from == killed_to == left == right == edges, case.name


def _homopolymer(case):
    order = b"ACGT"
    for s in case.segs:
        w = _scan(case, s.seq)["windows"]
        k = order.index(s.facts["base"])
        assert int(w["nucleotide_counts"][:, k].max()) >= B, s.name                    # a window holds the whole tile of it
        if s.facts["base"] in b"AT":
            assert len(_starts(case, s.seq)) >= B - 5 - 2 * (case.options().window_size == B)


def _windows(case):
    for sg in case.segs:
        f, n = sg.facts, sg.n
        w, s = f["w"], f["s"]
        recs = range(0, (n + s - 1) // s)
        if f.get("starts"):
            assert any(R > 0 and (R * s) % B == 0 for R in recs), sg.name
        if f.get("ends"):
            assert any(R * s + w <= n and (R * s + w) % B == 0 for R in recs), sg.name
        if f.get("tiles"):
            assert any(R * s + w <= n and (R * s + w - 1) // B - (R * s) // B + 1 >= f["tiles"] for R in recs), sg.name
        if f.get("not_multiple"):
            assert w % s != 0
        m = _starts(case, sg.seq)
        assert any(p < B <= p + l - 1 for p, l in m) or w == s, sg.name                # a match across the first tile boundary
        assert len(m) > 20, sg.name


def _capacity(case):
    (s,) = case.segs
    f = s.facts
    assert f["lo"] % 1024 == 0 and f["hi"] == f["lo"] + 1024 and f["lo"] // B == 1     # one wave's positions of the second tile
    inside = [p for p, l, _, _ in _matches(case, s.seq) if f["lo"] <= p < f["hi"]]
    assert len(inside) == f["candidates"] and len(inside) == len(_matches(case, s.seq)), case.name
    assert case.spills == (f["candidates"] > G.LIST_WAVE)
    assert min(inside) > f["lo"] + 32 and max(inside) < f["hi"] - 32


def _tips(case):
    t = G.TIPS_T
    offsets = set()
    for s in case.segs:
        m = _starts(case, s.seq)
        if s.n > 2 * t:
            assert all(p + l <= t or p >= s.n - t for p, l in m), s.name
            assert any(t - 18 <= p < t for p, l in m) and any(s.n - t <= p < s.n - t + 18 for p, l in m), s.name   # up to both inner ends
            offsets.add((s.n - t) % 16 == 0)
        else:
            assert any(p < t < p + l for p, l in m), s.name                             # one region: the copy across t is a match
        assert any(p < 60 for p, l in m) and any(p >= s.n - 60 for p, l in m), s.name
    assert offsets == {True, False}
    assert sorted({s.n for s in case.segs}) == [2 * t, 2 * t + 1, 2 * t + 15, 2 * t + 16, B + 2 * t]


FAMILY = dict(straddle=_straddle, halo_end=_halo_end, lengths=_lengths, invalid=_invalid, homopolymer=_homopolymer,
              windows=_windows, capacity=_capacity, tips=_tips)


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_case_is_what_it_claims(case):
    o = case.options()
    ambiguous = {p[0] for p in _oracle(case).patterns if len(p) > 3 and p[3]}
    for s in case.segs:
        got = _matches(case, s.seq)
        # every match is one the case planted (the C and G next to an array may complete its cut first or last unit)
        u = len(case.pset.unit) - 1
        planted = _merged(s.planted)
        for p, l, _, _ in got:
            assert any(a - u <= p and p + l <= b + u for a, b in planted), "%s: a match at %d (+%d) nobody planted" % (s.name, p, l)
        # and the oracle's list is the plain search's
        want = python_matches(case, s.seq)
        assert {(p, l) for p, l, _, _ in got} == set(want), s.name
        assert len(got) == len(want), s.name
        text = s.seq.upper() if case.fold else s.seq
        for p, l, f, c in got:
            if text[p:p + l].decode() not in ambiguous:
                assert (f, c) == want[(p, l)], "%s: flags of the match at %d (+%d)" % (s.name, p, l)
    assert np.all([len(s.planted) > 0 for s in case.segs])
    FAMILY[case.family](case)
