"""ts_bgzf_inflate without a GPU: the symbol is declared and exported, the ctypes mirrors have the C compiler's sizes, a
planning-only context answers TS_ERR_NO_DEVICE, and descriptors that point outside the buffers are refused on the host
(TS_ERR_INVALID_ARG) before any device is asked for."""
import ctypes as C
import os
import re
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planning():
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import parse_cli, user_input
    tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=K.DEVICE_NONE))
    yield tel
    tel.close() if hasattr(tel, "close") else None


def test_bgzf_symbols_declared_and_exported():
    from teloscope_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", hdr))
    assert "ts_bgzf_inflate" in declared and "ts_bgzf_inflate" in K.SYMBOLS
    lib = C.CDLL(K.LIB_PATH)
    assert hasattr(lib, "ts_bgzf_inflate")
    assert lib.ts_abi_version() == 4


def test_bgzf_struct_sizes_match_header(tmp_path):
    from teloscope_amd import _capi as K
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "teloscan.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu\\n", sizeof(ts_bgzf_block), sizeof(ts_bgzf_status), '
                   'offsetof(ts_bgzf_block, dst_off), offsetof(ts_bgzf_status, block));'
                   'printf("%d %d %d\\n", TS_BGZF_OK, TS_BGZF_BAD_DEFLATE, TS_BGZF_BAD_CRC);return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(K.BgzfBlock), C.sizeof(K.BgzfStatus), K.BgzfBlock.dst_off.offset, K.BgzfStatus.block.offset,
                   K.BGZF_OK, K.BGZF_BAD_DEFLATE, K.BGZF_BAD_CRC]
    assert got[:2] == [32, 16]
    src.write_text('#include <stdio.h>\n#include "teloscan.h"\nint main(void){printf("%zu\\n", sizeof(ts_bam_record));return 0;}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(K.BamRecord) == 24


def _member(plain):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = co.compress(plain) + co.flush()
    return payload, zlib.crc32(plain) & 0xFFFFFFFF


def test_planning_only_context_has_no_device(planning):
    from teloscope_amd import _capi as K
    from teloscope_amd.bgzf import inflate_blocks
    plain = b"TTAGGG" * 100
    payload, crc = _member(plain)
    with pytest.raises(K.TeloscanError) as ei:
        inflate_blocks(planning._ctx.ptr, payload, [(0, len(payload), len(plain), crc, 0)])
    assert ei.value.code == K.TS_ERR_NO_DEVICE
    assert "planning-only" in planning._ctx.error()


def test_bad_descriptors_are_refused_on_the_host(planning):
    """Every refusal below comes from a planning-only context: had a device been asked for, the answer would have been
    TS_ERR_NO_DEVICE."""
    from teloscope_amd import _capi as K
    from teloscope_amd.bgzf import inflate_blocks
    plain = b"ACGT" * 300
    payload, crc = _member(plain)
    n, m = len(payload), len(plain)
    ctx = planning._ctx.ptr
    bad = [
        [(1, n, m, crc, 0)],                                     # payload runs past the compressed bytes
        [(n + 1, 0, 0, 0, 0)],                                   # src_off beyond them
        [(2 ** 63, n, m, crc, 0)],                               # (no wrap-around)
        [(0, 65537, m, crc, 0)],                                 # payload_len above 64 KB
        [(0, n, 65537, crc, 0)],                                 # isize above 64 KB
        [(0, n, m, crc, 1)],                                     # output runs past plain_cap
        [(0, n, m, crc, 2 ** 64 - 4)],                           # (no wrap-around)
        [(0, n, m, crc, 0), (0, n, m, crc, m - 1)],              # outputs overlap
        [(0, n, m, crc, 5), (0, n, 10, crc, 0)],                 # ... in any order
    ]
    for blocks in bad:
        cap = m if len(blocks) == 1 else 2 * m - 1
        with pytest.raises(K.TeloscanError) as ei:
            inflate_blocks(ctx, payload, blocks, plain_cap=cap)
        assert ei.value.code == K.TS_ERR_INVALID_ARG, blocks
    L = K.lib()
    st = K.BgzfStatus()
    blk = (K.BgzfBlock * 1)()
    buf = C.create_string_buffer(16)
    assert L.ts_bgzf_inflate(None, buf, 16, blk, 1, buf, 16, C.byref(st)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bgzf_inflate(ctx, buf, 16, blk, 1, buf, 16, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_bgzf_inflate(ctx, None, 16, blk, 1, buf, 16, C.byref(st)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bgzf_inflate(ctx, buf, 16, None, 1, buf, 16, C.byref(st)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bgzf_inflate(ctx, buf, 16, blk, 1, None, 16, C.byref(st)) == K.TS_ERR_INVALID_ARG
    # touching empty outputs and an empty member between them do not overlap
    with pytest.raises(K.TeloscanError) as ei:
        inflate_blocks(ctx, payload, [(0, n, m, crc, 0), (0, 2, 0, 0, 7), (0, n, m, crc, m)], plain_cap=2 * m)
    assert ei.value.code == K.TS_ERR_NO_DEVICE


def test_bam_chunk_entry_points_without_a_device(planning):
    from teloscope_amd import _capi as K
    L = K.lib()
    ctx = planning._ctx.ptr
    assert not L.ts_bam_chunk_create(ctx, 1 << 20, 1 << 20)
    assert "planning-only" in planning._ctx.error()
    assert not L.ts_bam_chunk_create(None, 1 << 20, 1 << 20)
    assert not L.ts_bam_chunk_create(ctx, 0, 1 << 20)
    L.ts_bam_chunk_destroy(None)
    st = K.BgzfStatus()
    n = C.c_uint64(0)
    e = C.c_int(0)
    assert L.ts_bam_chunk_inflate(None, None, 0, None, 0, 0, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_chunk_status(None, C.byref(st)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_chunk_read(None, 0, 0, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_chunk_walk(None, 0, None, 0, C.byref(n), C.byref(n), C.byref(e), C.byref(n)) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_chunk_decode(None, None, 0, None, None) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_chunk_gather(None, None, 0, None, None, 0, C.byref(n), C.byref(n), None) == K.TS_ERR_INVALID_ARG
    assert L.ts_bam_chunk_size(None) == 0 and not L.ts_bam_chunk_pass_buffer(None, 16)
    assert C.sizeof(K.BamRecord) == 24


def test_bam_device_cli_builds_and_refuses_without_gpu(tmp_path):
    from teloscope_amd import _capi as K
    exe = tmp_path / "bam_device_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bam_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(exe)])
    if K.lib().ts_device_count() > 0:
        return                                                       # (with a GPU: tests/test_gpu_bam_device.py runs it)
    for route in ("--device", "--host"):
        r = subprocess.run([str(exe), "--bam-subset", route, "-"], stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
        assert r.returncode == 1 and b"no usable HIP device" in r.stderr, r.stderr
