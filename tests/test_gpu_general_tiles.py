"""The general kernels (generic.hip: list, position-strided and wide form) on the hand-built cases of tests/gentilecases.py
(proved on the host by tests/test_general_tile_cases_cpu.py): matches at every position around a tile boundary, a pattern on
the last halo base, segments that end one base either side of a tile, non-ACGT bytes on the edges, whole tiles of one base,
window records that start and end on tile boundaries or span several tiles, the largest geometry the list form takes, a
wave's candidate list at 1023 / 1024 / 1025 entries, and tips-only regions on and off a 16-byte offset.  One scan per case and
form, all of the case's segments in one call, bit-exact against the oracle; which form ran is read from the library's TS_TIMING
line and asserted for every table-form case; a forced single-length case must also equal the tiled route record for record."""
import re

import numpy as np
import pytest

from tests import gentilecases as G
from tests.backends import OracleBackend, assert_segment_equal, segment_as_dict

pytestmark = pytest.mark.gpu

CASES = G.CASES


def _abs_pos(i):
    """where segment i of a case lies in its path (the records' absolute positions start from it)"""
    return 1000003 * i


def _run(case, env, monkeypatch, capfd):
    """one scan_segments call of a fresh context made under `env` (+ TS_TIMING): (context, its patterns, results, stderr)"""
    import teloscope_amd as ta
    from teloscope_amd.cli import user_input
    opts = case.options()
    for k, v in env + (("TS_TIMING", "1"),):
        monkeypatch.setenv(k, v)
    try:
        ui = user_input(opts)
        ui.foldCase = case.fold
        tel = ta.Teloscope(ui)
    finally:
        for k, _ in env + (("TS_TIMING", "1"),):
            monkeypatch.delenv(k, raising=False)
    capfd.readouterr()
    got = [segment_as_dict(s) for s in tel.scanSegments([(s.seq, _abs_pos(i), opts.ultra_fast) for i, s in enumerate(case.segs)])]
    err = capfd.readouterr().err
    patterns = [(p, f, p in (opts.canonical_fwd, opts.canonical_rev)) for p, f in ui.patternInfo]
    return tel, patterns, got, err


def _assert_form(case, env, err):
    want = case.expected_form(env)
    assert "general path: route: %s form" % ("wide" if want == "wide" else "table") in err, (case.name, env, err[-2000:])
    forms = re.findall(r"fused pass: (\d+) groups in the list form, (\d+) in the strided form", err)
    assert forms, (case.name, env, err[-2000:])
    n_list, n_strided = sum(int(a) for a, _ in forms), sum(int(b) for _, b in forms)
    if want == "list":                      # every group ended in the list form: none spilled, none fell back
        assert n_list > 0 and n_strided == 0, (case.name, env, forms)
    else:
        assert n_list == 0 and n_strided > 0, (case.name, env, forms)


def _same(a, b, ctx):
    """two SegmentData dicts of the product, field for field"""
    assert sorted(a) == sorted(b)
    for name in a:
        x, y = a[name], b[name]
        assert len(x) == len(y) and x.dtype == y.dtype, "%s %s: %d vs %d records" % (ctx, name, len(x), len(y))
        for f in x.dtype.names:
            if x.dtype[f].kind == "f":
                assert np.array_equal(x[f], y[f], equal_nan=True), "%s %s.%s differs" % (ctx, name, f)
            else:
                assert np.array_equal(x[f], y[f]), "%s %s.%s differs" % (ctx, name, f)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_matches_the_oracle_in_every_form(case, monkeypatch, capfd):
    opts = case.options()
    tips = opts.ultra_fast
    orac = OracleBackend(opts)
    expected, forced = None, None
    for env in case.forms:
        tel, patterns, got, err = _run(case, env, monkeypatch, capfd)
        assert not tel.usesFastPath(), (case.name, env)
        _assert_form(case, env, err)
        if expected is None:
            if orac.ambiguous:
                orac = orac.with_ambiguous_orientation_from(patterns)
            expected = [orac.scan_segment(s.seq.upper() if case.fold else s.seq, _abs_pos(i), tips) for i, s in enumerate(case.segs)]
        for s, g, e in zip(case.segs, got, expected):
            assert_segment_equal(g, e, tips, ctx="case %s form %s segment %s:" % (case.name, dict(env) or "default", s.name))
        if forced is None:
            forced = got
    if case.tiled_twin:
        tel, _, got, err = _run(case, G.NO_ENV, monkeypatch, capfd)
        assert tel.usesFastPath() and "general path" not in err, (case.name, err[-2000:])
        for s, g, f, e in zip(case.segs, got, forced, expected):
            _same(f, g, "case %s segment %s: general against tiled:" % (case.name, s.name))
            assert_segment_equal(g, e, tips, ctx="case %s tiled route segment %s:" % (case.name, s.name))
    else:
        assert not case.pset.forced or case.family == "windows", case.name
