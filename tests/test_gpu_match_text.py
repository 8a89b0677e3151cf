"""ts_match_lines_format — the device match-line formatter by itself (match_text.hip) — against tests/matchtext.py, byte for
byte: the generated record list the host program formats on the CPU (tests/test_match_format_core_cpu.py: every digit count of
position and end, sizes 1 to 63, names of 1 to 300 bytes, mixed-case bases, the edges of the terminal rule), segments of 0, 1, 63,
64, 65 and 200 records (a wave's and a pseudo-tile's worth of lines crossed), records skipped between segments, names beyond the
staging area, a tips-only segment, no records at all, a context without -m, a struct reused across calls, text that leaves the
device in several slices, and what the entry point refuses."""
import ctypes as C

import pytest

from tests import matchtext as M
from tests.test_gpu_input_device import make

pytestmark = pytest.mark.gpu

CLI = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -m -t %d" % M.CASE_LIMIT


@pytest.fixture(scope="module")
def tel():
    _, t = make(CLI)
    yield t
    t.close()


def stats(tel):
    from teloscope_amd import _capi as K
    s = (C.c_uint64 * 4)()
    assert K.lib().ts_match_text_stats(tel._ctx.ptr, s) == K.TS_OK
    return [int(x) for x in s]


def check(tel, records, segs, bases, text=None):
    want, want_lines = M.format_matches(records, segs, bases, M.CASE_LIMIT)
    before = stats(tel)
    got, lines = M.device_format(tel, records, segs, bases, text)
    assert lines == want_lines
    for f in range(M.N_FILES):
        assert got[f] == want[f], "file %d differs" % f
    after = stats(tel)
    assert after[1] - before[1] == want_lines[0] and after[2] - before[2] == want_lines[1]
    assert after[3] - before[3] == len(want[0]) + len(want[1])
    return got, lines


def test_the_host_programs_record_list(tel):
    records, segs, bases = M.generated_case()
    got, lines = check(tel, records, segs, bases)
    assert lines[0] > 100 and 0 < lines[1] < lines[0]
    assert b"\t18446744073709551609\t18446744073709551615\t" in got[0]          # 2^64 - 1 as an end
    assert b"\t9999999997\t10000000003\t" in got[0]


@pytest.mark.parametrize("long_name", [False, True], ids=["short names", "names beyond the staging area"])
def test_segments_of_0_1_63_64_65_200_records(tel, long_name):
    records, segs, bases = M.counted_case([0, 1, 63, 64, 65, 200, 0, 513, 1024, 3], long_name=long_name)
    check(tel, records, segs, bases)


def test_records_skipped_between_segments_and_a_tips_only_segment(tel):
    records, segs, bases = M.counted_case([70, 5, 130])
    # segment 1 becomes tips-only; records 40..69 of segment 0 belong to nobody
    segs[0] = (0, 40) + segs[0][2:]
    segs[1] = segs[1][:6] + (True,)
    got, lines = check(tel, records, segs, bases)
    assert b"seq1\t" not in got[0] + got[1] and lines[0] > 0


def test_zero_records_and_zero_segments(tel):
    assert check(tel, [], [], b"") == ([b"", b""], [0, 0])
    records, segs, bases = M.counted_case([0, 0])
    assert check(tel, records, segs, bases) == ([b"", b""], [0, 0])


def test_a_context_without_m_gives_no_text():
    from teloscope_amd import _capi as K
    _, t = make("-w 1000 -s 500 -r -t %d" % M.CASE_LIMIT)
    try:
        records, segs, bases = M.counted_case([10])
        got, lines = M.device_format(t, records, segs, bases)
        assert got == [None, None] and lines == [0, 0]
        s = (C.c_uint64 * 4)()
        assert K.lib().ts_match_text_stats(t._ctx.ptr, s) == K.TS_OK and list(s) == [0, 0, 0, 0]
    finally:
        t.close()


def test_a_struct_reused_across_calls_of_different_size(tel):
    from teloscope_amd import _capi as K
    text = K.MatchText()
    try:
        big = M.counted_case([300, 200])
        small = M.counted_case([3], seed=9)
        check(tel, *big, text=text)
        cap = [int(text.capacity[f]) for f in range(M.N_FILES)]
        ptr = [text.text[f] for f in range(M.N_FILES)]
        check(tel, *small, text=text)                                  # replaced, not appended; the arrays are kept
        assert [int(text.capacity[f]) for f in range(M.N_FILES)] == cap and [text.text[f] for f in range(M.N_FILES)] == ptr
        check(tel, *M.counted_case([900, 700]), text=text)              # grown
        assert all(int(text.capacity[f]) >= int(text.len[f]) for f in range(M.N_FILES))
        check(tel, [], [], b"", text=text)
        assert [int(text.len[f]) for f in range(M.N_FILES)] == [0, 0] and all(text.text[f] for f in range(M.N_FILES))
    finally:
        K.lib().ts_free_match_text(C.byref(text))
    assert all(not text.text[f] and text.capacity[f] == 0 for f in range(M.N_FILES))


def test_text_that_leaves_in_several_slices(tel, monkeypatch):
    """TS_MATCH_SLICE_BYTES=4096: the two files go through in runs of pseudo-tiles of at most 4 KiB (a tile beyond it alone)."""
    from teloscope_amd import _capi as K
    records, segs, bases = M.counted_case([3000, 0, 700, 64, 2000], long_name=True)
    monkeypatch.setenv("TS_MATCH_SLICE_BYTES", "4096")
    assert K.lib().ts_refresh_env(tel._ctx.ptr) == K.TS_OK
    try:
        got, _ = check(tel, records, segs, bases)
        assert len(got[0]) > 20 * 4096
    finally:
        monkeypatch.delenv("TS_MATCH_SLICE_BYTES")
        assert K.lib().ts_refresh_env(tel._ctx.ptr) == K.TS_OK
    check(tel, records, segs, bases)


def test_what_the_entry_point_refuses(tel):
    from teloscope_amd import _capi as K
    records, segs, bases = M.counted_case([4])
    cases = {
        "a record in front of its segment": ([(segs[0][2] + 5, 6, 2)], [(0, 1, segs[0][2] + 10, 100, 0, b"x", False)]),
        "a record that ends behind its segment": ([(95, 6, 2)], [(0, 1, 0, 100, 0, b"x", False)]),
        "size 0": ([(5, 0, 2)], [(0, 1, 0, 100, 0, b"x", False)]),
        "size 64": ([(5, 64, 2)], [(0, 1, 0, 100, 0, b"x", False)]),
        "records beyond the array": ([(5, 6, 2)], [(0, 2, 0, 100, 0, b"x", False)]),
        "overlapping segments": ([(5, 6, 2), (6, 6, 2)], [(0, 2, 0, 100, 0, b"x", False), (1, 1, 0, 100, 0, b"y", False)]),
        "bases outside the bases": ([(5, 6, 2)], [(0, 1, 0, len(bases) + 1, 0, b"x", False)]),
    }
    for what, (recs, table) in cases.items():
        with pytest.raises(K.TeloscanError) as e:
            M.device_format(tel, recs, table, bases)
        assert e.value.code == K.TS_ERR_INVALID_ARG, what
    check(tel, records, segs, bases)                                    # the context is fine afterwards


def test_runs_of_64_lines_start_at_every_residue_mod_16(tel):
    """17 segments of 65 records with names of 1 to 16 bytes: a segment is one pseudo-tile, whose records a wave takes in runs of
    64, and the lines of such a run start on every residue modulo 16 of their file (a file's block starts 256-byte aligned) —
    checked on the reference text before the device is asked — so the copy-out (text_store_core.h) meets every shift."""
    records, segs, bases = M.counted_case([65] * 17)
    # (the name lengths in an order in which the 51 run starts do reach every residue: in ascending order they miss one)
    name_lens = [1, 5, 16, 7, 10, 14, 11, 6, 9, 2, 15, 3, 4, 8, 12, 13, 7]
    segs = [sg[:5] + (bytes(97 + (i + k) % 26 for k in range(name_lens[i])),) + sg[6:] for i, sg in enumerate(segs)]
    assert {len(sg[5]) for sg in segs} == set(range(1, 17))
    want, _ = M.format_matches(records, segs, bases, M.CASE_LIMIT)
    at, residues, pieces = [0, 0], set(), [[], []]
    for sg in segs:
        for i0 in range(0, sg[1], 64):
            run, _ = M.format_matches(records, [(sg[0] + i0, min(64, sg[1] - i0)) + sg[2:]], bases, M.CASE_LIMIT)
            for f in range(M.N_FILES):
                if run[f]:
                    residues.add(at[f] % 16)
                    pieces[f].append(run[f])
                    at[f] += len(run[f])
    assert [b"".join(p) for p in pieces] == want                       # (the runs are the text, cut where the waves cut it)
    assert residues == set(range(16))
    check(tel, records, segs, bases)
