"""TS_INPUT_DEVICE through ctypes: segments whose bases already lie in device memory give, byte for byte, what the same bases
give as TS_INPUT_BASES — and what the oracle computes — for full and tips-only scans on the tiled kernel, a list-form and a
wide-form pattern set, through ts_scan_segments, ts_scan_segments_blocks and ts_terminal_ends; mixed with host segments, at odd
device addresses, for the shortest lengths and for a segment longer than a pipeline group."""
import ctypes as C

import numpy as np
import pytest

from tests import bamchunk as B
from tests import harness as H
from tests import seqgen
from tests.backends import OracleBackend, assert_segment_equal, segment_as_dict
from tests.test_gpu_parity import WIDE_GRID

pytestmark = pytest.mark.gpu

HEADLINE = "-c TTAGGG -p TTAGGG,TCAGGG,TGAGGG,TTGGGG -w 1000 -s 500 -r -g -e -m -i"
LIST_FORM = "-p TTAGGG,TTAGG -w 1000 -s 500 -r -g -e -m -i"
SETS = {"tiled": HEADLINE, "list": LIST_FORM, "wide": WIDE_GRID[1]}


class DeviceBytes:
    """Bytes in device memory, `shift` bytes behind a 256-byte aligned allocation."""

    def __init__(self, data, shift=0):
        self.hip = B.hip()
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.base = C.c_void_p(0)
        assert self.hip.hipMalloc(C.byref(self.base), len(data) + shift + 64) == 0
        self.ptr = self.base.value + shift
        if len(data):
            B.to_device(self.ptr, data)

    def free(self):
        if self.base:
            assert self.hip.hipFree(self.base) == 0
            self.base = None


def make(cli):
    import teloscope_amd as ta
    from teloscope_amd.cli import user_input
    opts = H.parse_cli("x.fa " + cli)
    return opts, ta.Teloscope(user_input(opts, device=0))


def segments_in(K, specs, keep):
    """specs: [(bytes, abs_pos, tips, on_device, shift)] -> a ts_segment_in array; device copies are appended to keep."""
    arr = (K.SegmentIn * max(1, len(specs)))()
    for i, (seq, abs_pos, tips, on_device, shift) in enumerate(specs):
        if on_device:
            d = DeviceBytes(seq, shift)
            keep.append(d)
            arr[i].seq = d.ptr                                  # (a c_char_p field takes an address)
            arr[i].input_format = K.TS_INPUT_DEVICE
        else:
            keep.append(seq)
            arr[i].seq = seq
        arr[i].len, arr[i].abs_pos, arr[i].tips_only = len(seq), abs_pos, int(tips)
    return arr


def scan(tel, specs, blocks=False):
    """-> [SegmentData] (+ counts when blocks) of one call"""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    keep, n = [], len(specs)
    arr = segments_in(K, specs, keep)
    out = (K.SegmentOut * max(1, n))()
    try:
        if blocks:
            cnt = (K.SegmentCounts * max(1, n))()
            rc = K.lib().ts_scan_segments_blocks(tel._ctx.ptr, arr, n, out, cnt)
        else:
            rc = K.lib().ts_scan_segments(tel._ctx.ptr, arr, n, out)
        assert rc == K.TS_OK, tel._ctx.error()
        res = [ta.SegmentData(out[i], bool(specs[i][2])) for i in range(n)]
        K.lib().ts_free_segments(out, n)
        if blocks:
            return res, [(c.n_windows, c.n_matches, c.n_canonical, c.n_forward) for c in cnt[:n]]
        return res
    finally:
        for k in keep:
            if isinstance(k, DeviceBytes):
                k.free()


def assert_bytes_equal(got, exp, what):
    for g, e, in zip(got, exp):
        for name in ("windows", "terminalBlocks", "interstitialBlocks", "_m"):
            assert getattr(g, name).tobytes() == getattr(e, name).tobytes(), "%s: %s differ" % (what, name)


def on_device(specs, which=None):
    return [(s, a, t, which is None or i in which, sh) for i, (s, a, t, _, sh) in enumerate(specs)]


@pytest.fixture(scope="module")
def sequences():
    rng = np.random.default_rng(20261017)
    return [seqgen.chromosome(rng, n, n_its=3, iupac=3, lower=0.05) for n in (70_001, 33_333, 9_999)]


@pytest.mark.parametrize("name", sorted(SETS))
def test_device_segments_equal_host_segments_and_the_oracle(name, sequences):
    """Full and tips-only scans in one call, every segment at an odd device address; the third set of segments mixes both forms."""
    opts, tel = make(SETS[name] + " -t 3000")
    orac = OracleBackend(opts)
    specs = []
    for i, s in enumerate(sequences):
        specs.append((s, 100 * i, False, False, 1 + 2 * i))
        specs.append((s, 7 + i, True, False, 3 + 4 * i))       # (longer than twice the terminal limit: two regions per segment)
    host = scan(tel, specs)
    for what, sel in (("all on the device", None), ("mixed", {0, 3, 4})):
        dev = scan(tel, on_device(specs, sel))
        assert_bytes_equal(dev, host, "%s, %s" % (name, what))
    if orac.ambiguous:
        from tests.backends import ProductBackend
        orac = orac.with_ambiguous_orientation_from(ProductBackend(opts).patterns)
    dev = scan(tel, on_device(specs))
    for (s, a, t, _, _), d in zip(specs, dev):
        # (the oracle is strict scanSegment, lower case = non-ACGT: a context that folds case sees the upper-cased bases)
        assert_segment_equal(segment_as_dict(d), orac.scan_segment(s.upper(), a, t), t, ctx="%s abs %d tips %d" % (name, a, t))
    # the blocks-only entry and its counts
    hb, hc = scan(tel, specs, blocks=True)
    db, dc = scan(tel, on_device(specs, {1, 2, 5}), blocks=True)
    assert_bytes_equal(db, hb, name + ", blocks only")
    assert dc == hc
    tel.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_shortest_lengths(name):
    rng = np.random.default_rng(5)
    opts, tel = make(SETS[name])
    specs = []
    for n in (0, 1, 15, 16, 17):
        s = (b"TTAGGG" * 4)[:n] if n % 2 else bytes(rng.choice(list(b"ACGTN"), n).astype(np.uint8))
        specs.append((s, n, False, False, n % 5))
        specs.append((s, n, True, False, 1))
    host = scan(tel, specs)
    assert_bytes_equal(scan(tel, on_device(specs)), host, name + ", short")
    assert_bytes_equal(scan(tel, on_device(specs, {0, 1, 4, 9})), host, name + ", short and mixed")
    tel.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_terminal_ends(name, sequences):
    from teloscope_amd import _capi as K
    opts, tel = make(SETS[name] + " -t 3000")
    specs = [(s, 0, True, False, 1 + i) for i, s in enumerate(sequences)] + [(b"", 0, True, False, 0), (b"CCCTAA" * 200, 0, True, False, 5)]
    want = tel.terminalEnds([s[0] for s in specs])
    keep = []
    arr = segments_in(K, on_device(specs, {0, 2, 3, 4}), keep)
    ends = np.zeros((len(specs), 2), dtype=np.uint32)
    rc = K.lib().ts_terminal_ends(tel._ctx.ptr, arr, len(specs), ends.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == K.TS_OK, tel._ctx.error()
    assert np.array_equal(ends, want)
    assert want.any() or name == "wide"                         # (that set's patterns, TTA + A..., call no block on these ends)
    for k in keep:
        if isinstance(k, DeviceBytes):
            k.free()
    tel.close()


def test_segment_longer_than_a_group():
    """A device segment of more than the 512 MiB a pipeline group holds, beside a small host segment: windows, blocks and counts
    equal those of the same bases from host memory."""
    rng = np.random.default_rng(9)
    unit = seqgen.chromosome(rng, 1 << 20, n_its=4, iupac=2)
    big = unit * 513 + b"ACGTN" * 7
    assert len(big) > 512 << 20
    opts, tel = make(HEADLINE)
    specs = [(big, 0, False, False, 3), (unit[:50_001], 5, False, False, 0)]
    hb, hc = scan(tel, specs, blocks=True)
    db, dc = scan(tel, on_device(specs, {0}), blocks=True)
    assert_bytes_equal(db, hb, "longer than a group")
    assert dc == hc and hc[0][0] == (len(big) + 499) // 500
    tel.close()


def test_multi_refuses_device_segments(sequences):
    from teloscope_amd import _capi as K
    opts, tel = make(HEADLINE)
    _, tel2 = make(HEADLINE)
    keep = []
    arr = segments_in(K, [(sequences[0], 0, False, False, 0), (sequences[1], 0, False, True, 0)], keep)
    out = (K.SegmentOut * 2)()
    ctxs = (C.c_void_p * 2)(tel._ctx.ptr, tel2._ctx.ptr)
    assert K.lib().ts_scan_segments_multi(ctxs, 2, arr, 2, out, None) == K.TS_ERR_INVALID_ARG
    msg = tel._ctx.error()
    assert "TS_INPUT_DEVICE" in msg and "one device" in msg
    arr[1].input_format = 4
    assert K.lib().ts_scan_segments_multi(ctxs, 2, arr, 2, out, None) == K.TS_ERR_INVALID_ARG
    assert tel._ctx.error() == "unknown input_format"
    assert K.lib().ts_scan_segments(tel._ctx.ptr, arr, 2, out) == K.TS_ERR_INVALID_ARG
    assert tel._ctx.error() == "unknown input_format"
    assert K.lib().ts_abi_version() == 4 and K.TS_INPUT_DEVICE == 3
    for k in keep:
        if isinstance(k, DeviceBytes):
            k.free()
    tel.close()
    tel2.close()
