"""The three entry points of the per-side maxima on the device — ts_batch_terminal_ends, ts_terminal_ends_stats and their
mirrors — are declared, exported and bound; the ABI version has not moved.  No device is needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_terminal_ends_calls():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+ts_batch_terminal_ends\(ts_batch \*b, void \*d_ends, void \*stream\);", bare)
    assert re.search(r"int\s+ts_terminal_ends_stats\(const ts_ctx \*ctx, uint64_t out\[4\]\);", bare)
    assert re.search(r"int\s+ts_terminal_ends\(ts_ctx \*ctx, const ts_segment_in \*segs, size_t n_segs, uint32_t \*ends\);", bare)
    assert "#define TELOSCAN_ABI_VERSION 4" in hdr and K.lib().ts_abi_version() == 4
    for name in ("ts_batch_terminal_ends", "ts_terminal_ends_stats", "ts_terminal_ends"):
        assert name in K.SYMBOLS and getattr(K.lib(), name).argtypes is not None, name
    assert "terminalEndsStats()" in open(os.path.join(ROOT, "include", "teloscope_mi355x.hpp")).read()
    assert callable(ta.Teloscope.terminal_ends_stats)
    assert K.lib().ts_terminal_ends_stats(None, None) == K.TS_ERR_INVALID_ARG
    assert K.lib().ts_batch_terminal_ends(None, None, None) == K.TS_ERR_INVALID_ARG
