"""The plain blocks the deflate encoder (teloscope_amd/csrc/deflate_core.h) is tested on, and the host program that runs the
core on them (tests/cpp/deflate_core_host.cpp): shared by tests/test_deflate_core_cpu.py, which builds the program under
sanitizers, and the GPU tests, which compare the device's payloads with the program's byte for byte."""
import os
import struct
import subprocess
import zlib

import numpy as np

from tests.test_inflate_core_cpu import contents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BLOCK = 0xFF00
# below and at the hashed length, batch edges, the longest match, the distance limit, the largest block
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 257, 258, 259, 260, 32767, 32768, 32769, 65279, 65280]
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def fibonacci_block():
    """46 367 bytes whose byte counts are F1..F22: an unlimited Huffman code of them is 21 bits deep."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = np.repeat(np.arange(22, dtype=np.uint8) + 40, fib)
    assert len(data) == 46367
    np.random.default_rng(77).shuffle(data)
    return data.tobytes()


def named_blocks():
    """[(name, plain)]: every kind of content at every size of SIZES, then the special blocks."""
    rng = np.random.default_rng(2024)
    data, far = contents(rng)
    data["noise"] = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    out = [("%s:%d" % (kind, n), v[:n]) for kind, v in data.items() for n in SIZES]
    noise = data["noise"][:32768]
    out.append(("far_exact", far))                                             # the repeat is 32 768 back
    out.append(("far_plus1", noise + b"\x00" + noise[:30000]))                 # 32 769 back: no match may reach it
    out.append(("fibonacci", fibonacci_block()))
    out.append(("two_bytes", bytes(rng.integers(0, 2, 5000, dtype=np.uint8) * 7 + 3)))
    out.append(("two_bytes_apart", b"ab" * 2 + b"a"))
    out.append(("chain", b"abcdefg" * 9000))                                   # one long chain of matches
    # the block's first bytes again at its start: a source in front of the block would serve them
    for lead in (1, 3, 4, 5, 64, 258):
        head = data["noise"][40000:40000 + lead]
        out.append(("front:%d" % lead, head * 3 + data["qual"][:200] + head))
    return out


def build_host_encoder(directory, sanitize):
    """Compiles tests/cpp/deflate_core_host.cpp into `directory`; returns run(blocks, tag) -> [(payload, crc)] and
    lengths(cases, tag) -> [bytes].  Any output on stderr fails the run."""
    exe = os.path.join(str(directory), "deflate_core_host")
    src = os.path.join(ROOT, "tests", "cpp", "deflate_core_host.cpp")
    base = ["g++", "-std=c++17", "-g", src, "-o", exe]
    base += ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    empty = os.path.join(str(directory), "empty.blocks")
    with open(empty, "wb") as f:
        f.write(struct.pack("<I", 0))
    for extra in ([], ["-static-libasan"]) if sanitize else ([],):  # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + extra)
        r = subprocess.run([exe, empty, empty + ".out"], capture_output=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def start(args):
        r = subprocess.run([exe] + args, capture_output=True, timeout=1200, env=env)
        assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]

    def run(blocks, tag):
        fin, fout = os.path.join(str(directory), tag + ".blocks"), os.path.join(str(directory), tag + ".out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(blocks)))
            for plain in blocks:
                f.write(struct.pack("<I", len(plain)) + plain)
        start([fin, fout])
        with open(fout, "rb") as f:
            raw = f.read()
        out, at = [], 0
        for _ in blocks:
            m, crc = struct.unpack_from("<II", raw, at)
            out.append((raw[at + 8:at + 8 + m], crc))
            at += 8 + m
        assert at == len(raw)
        return out

    def lengths(cases, tag):
        fin, fout = os.path.join(str(directory), tag + ".cases"), os.path.join(str(directory), tag + ".out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for limit, counts in cases:
                f.write(struct.pack("<II%dI" % len(counts), len(counts), limit, *counts))
        start(["--lengths", fin, fout])
        with open(fout, "rb") as f:
            raw = f.read()
        out, at = [], 0
        for _, counts in cases:
            out.append(raw[at:at + len(counts)])
            at += len(counts)
        assert at == len(raw)
        return out

    run.lengths = lengths
    return run


class Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def dynamic_header(payload):
    """The code lengths a BTYPE 2 block announces: (code-length code's lengths [19], literal/length lengths, distance lengths)."""
    b = Bits(payload)
    assert b.take(1) == 1 and b.take(2) == 2
    nl, nd, nc = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    clen = [0] * 19
    for i in range(nc):
        clen[ORDER[i]] = b.take(3)
    # canonical decode of the code-length code
    codes, code = {}, 0
    for length in range(1, 8):
        for s in range(19):
            if clen[s] == length:
                codes[(length, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < nl + nd:
        code, length = 0, 0
        while (length, code) not in codes:
            code = code << 1 | b.take(1)
            length += 1
            assert length <= 7
        s = codes[(length, code)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.take(2))
        elif s == 17:
            lens += [0] * (3 + b.take(3))
        else:
            lens += [0] * (11 + b.take(7))
    assert len(lens) == nl + nd
    return clen, lens[:nl], lens[nl:]


def kraft(lens):
    """Sum of 2^-l over the used lengths, in units of 2^-15."""
    return sum(1 << (15 - l) for l in lens if l)


def raw_inflate(payload):
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    assert d.eof and not d.unused_data
    return out
