"""BGZF members inflated on the device (ts_bgzf_inflate of include/teloscan.h): the caller locates the members, the GPU
decodes and checksums them, a wave per member.  There is no host decoder behind this.  deflate_blocks is the other direction
(ts_bgzf_deflate): plain bytes in, complete members out, compressed by a wave per member; no zlib behind it either."""
import ctypes as C

import numpy as np

from . import _capi as K

BLOCK_DT = np.dtype(K.BgzfBlock)


def inflate_blocks(ctx, data, blocks, plain_cap=None):
    """data: the compressed bytes; blocks: (src_off, payload_len, isize, crc, dst_off) per member, or an array of BLOCK_DT;
    ctx: a context pointer (Teloscope._ctx.ptr).  -> (plain bytes of plain_cap, (code, block)): code is BGZF_OK, or what is
    wrong with the lowest member that is not ok, and block is its index (len(blocks) when all are ok)."""
    if isinstance(blocks, np.ndarray) and blocks.dtype == BLOCK_DT:
        arr = np.ascontiguousarray(blocks)
    else:
        arr = np.zeros(len(blocks), dtype=BLOCK_DT)
        for i, (src_off, payload_len, isize, crc, dst_off) in enumerate(blocks):
            arr[i] = (src_off, payload_len, isize, crc, 0, dst_off)
    if plain_cap is None:
        plain_cap = int((arr["dst_off"] + arr["isize"]).max()) if len(arr) else 0
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(max(1, plain_cap), dtype=np.uint8)
    status = K.BgzfStatus()
    rc = K.lib().ts_bgzf_inflate(ctx, src.ctypes.data if len(src) else None, len(src),
                                 arr.ctypes.data_as(C.POINTER(K.BgzfBlock)) if len(arr) else None, len(arr),
                                 out.ctypes.data if plain_cap else None, plain_cap, C.byref(status))
    if rc != K.TS_OK:
        msg = K.lib().ts_last_error(ctx)
        raise K.TeloscanError(rc, msg.decode() if msg else "ts_bgzf_inflate failed")
    return out[:plain_cap].tobytes(), (int(status.code), int(status.block))


def deflate_blocks(ctx, data, payload_bytes=0xFF00):
    """data: plain bytes, cut into consecutive payloads of payload_bytes (1 .. 65280); ctx: a context pointer.  -> the BGZF
    members, one per payload, concatenated (no EOF marker; b"" for no data)."""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    members = -(-len(src) // payload_bytes) if 0 < payload_bytes <= 0xFF00 else 0
    out = np.zeros(max(1, len(src) + 31 * members), dtype=np.uint8)      # (a payload grows by 5 bytes at most, plus 26 of framing)
    nbytes, count = C.c_uint64(0), C.c_uint64(0)
    rc = K.lib().ts_bgzf_deflate(ctx, src.ctypes.data if len(src) else None, len(src), payload_bytes, out.ctypes.data, len(out),
                                 C.byref(nbytes), C.byref(count))
    if rc != K.TS_OK:
        msg = K.lib().ts_last_error(ctx)
        raise K.TeloscanError(rc, msg.decode() if msg else "ts_bgzf_deflate failed")
    return out[:nbytes.value].tobytes()
