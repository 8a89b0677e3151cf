"""Plain gzip through detail::ChunkFeed's Gzip source on the GPU (tests/cpp/gzip_device_cli.cpp: the feed the three text routes
read from, without a route around it): ts_gzip_decode, ts_gzip_take into the resident chunk, member headers and trailers on
the host, and zlib wherever the device's chain of blocks stops short.  The odd files: two members, a member of header and
trailer only, a level-0 file, one letter a million times, noise, and 200 damaged copies of one file, each against
zlib.decompressobj(31).  tests/test_gzip_core_cpu.py runs the same decoder and the same host logic under sanitizers, so that
file comes first in any job that runs this one.  These are ordinary damaged inputs, as in tests/test_gpu_bgzf.py: the decoder's
bounds are what is under test, and none of them is meant to make the device fault."""
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from tests import gziptexts as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    out = tmp_path_factory.mktemp("cpp") / "gzip_device_cli"
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gzip_device_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def env(span=4096, window=8 << 20, device=1, min_bytes=0):
    return dict(os.environ, TS_GZIP_DEVICE=str(device), TS_GZIP_SPAN=str(span), TS_GZIP_WINDOW=str(window), TS_GZIP_MIN_BYTES=str(min_bytes))


def feed(cli, path, want=1 << 20, **kw):
    r = subprocess.run([cli, str(path), str(want)], capture_output=True, timeout=120, env=env(**kw))
    assert r.returncode in (0, 1), r.stderr[-500:]
    last = r.stderr.decode().splitlines()[-1]
    stats = dict(kv.split("=") for kv in last.split()) if r.returncode == 0 else {}
    return r.returncode, r.stdout, {k: int(v) for k, v in stats.items()}, last


def gz(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def test_clean_file_comes_from_the_device(cli, tmp_path):
    """The test that fails without the feature: the bytes are right AND the device produced all of them."""
    plain = G.text("fastq", 1_200_000)
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(G.gzip_file("fastq", 1_200_000, 6))
    for span, window, want in ((4096, 8 << 20, 1 << 20), (32768, 200_000, 4096), (16384, 8 << 20, 77_777)):
        rc, out, s, last = feed(cli, p, want=want, span=span, window=window)
        assert rc == 0 and out == plain, last
        assert s["source"] == 3 and s["device_bytes"] == len(plain) and s["zlib_parts"] == 0 and s["chained"] >= 4, last
    rc, out, s, last = feed(cli, p, device=0)
    assert rc == 0 and out == plain and s["source"] == 2 and s["windows"] == 0, last      # TS_GZIP_DEVICE=0: a Stream through zlib
    rc, out, s, last = feed(cli, p, min_bytes=1 << 20)
    assert rc == 0 and out == plain and s["source"] == 2 and s["windows"] == 0, last      # smaller than the threshold: zlib


def test_two_members_and_an_empty_one(cli, tmp_path):
    a, b = G.text("fasta", 400_000), G.text("gfa", 300_000)
    p = tmp_path / "two.gz"
    p.write_bytes(gz(a, 9) + gz(b"") + gz(b, 1) + b"trailing bytes that are no member")
    rc, out, s, last = feed(cli, p, span=4096)
    assert rc == 0 and out == a + b, last
    assert s["device_bytes"] == len(a) + len(b), last
    p.write_bytes(gz(b""))
    rc, out, s, last = feed(cli, p)
    assert rc == 0 and out == b"" and s["device_bytes"] == 0, last


def test_level0_file_goes_through_zlib(cli, tmp_path):
    plain = G.text("gfa", 600_000)
    p = tmp_path / "stored.gz"
    p.write_bytes(gz(plain, 0))
    rc, out, s, last = feed(cli, p, span=4096, window=200_000)
    assert rc == 0 and out == plain, last
    # stored blocks only: no candidate in any window, zlib reads everything, and the statistics say so
    assert s["device_bytes"] == 0 and s["chained"] == 0 and s["zlib_parts"] >= 3 and s["windows"] >= 3, last


def test_one_letter_a_million_times(cli, tmp_path):
    plain = b"A" * 1_000_000 + G.text("fastq", 300_000)
    p = tmp_path / "one.gz"
    p.write_bytes(gz(plain))
    rc, out, s, last = feed(cli, p, span=4096)
    assert rc == 0 and out == plain, last
    # the letter's blocks hold more than a span has room for: the chain stops there, zlib takes over, the device resumes
    assert s["zlib_parts"] >= 1 and s["device_bytes"] >= 100_000, last


def test_noise(cli, tmp_path):
    plain = np.random.default_rng(5).integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    p = tmp_path / "noise.gz"
    p.write_bytes(gz(plain))
    rc, out, s, last = feed(cli, p, span=4096, window=100_000)
    assert rc == 0 and out == plain, last


def test_damaged_copies_get_zlibs_verdict(cli, tmp_path):
    """200 damaged copies of one 300 KB file, through one process: single bit flips behind the header and truncations.  Each
    gets zlib's verdict and, where zlib accepts (a truncated file: what it could still produce), zlib's bytes."""
    good = G.gzip_file("fastq", 300_000, 6)
    rng = random.Random(2024)
    names, want = [], {}
    for i in range(200):
        bad = bytearray(good)
        if i % 2 == 0:
            at = rng.randrange(80, 8 * len(bad))
            bad[at // 8] ^= 1 << (at % 8)
        else:
            del bad[rng.randrange(10, len(bad)):]
        p = tmp_path / ("bad%03d.gz" % i)
        p.write_bytes(bytes(bad))
        names.append(p)
        d = zlib.decompressobj(31)
        try:
            want[p] = d.decompress(bytes(bad))
        except zlib.error:
            want[p] = None
    lst = tmp_path / "list.txt"
    lst.write_text("".join(str(p) + "\n" for p in names))
    r = subprocess.run([cli, "--each", str(lst), "65536"], capture_output=True, timeout=300, env=env(span=4096, window=100_000))
    assert r.returncode == 0, r.stderr[-500:]
    verdicts = {True: 0, False: 0}
    for p in names:
        ok = os.path.exists(str(p) + ".ok")
        assert ok != os.path.exists(str(p) + ".err"), p
        assert ok == (want[p] is not None), (p.name, open(str(p) + ".err").read() if not ok else "accepted")
        if ok:
            assert open(str(p) + ".out", "rb").read() == want[p], p.name
        else:
            assert open(str(p) + ".err").read().strip() == "cannot read", p.name
        verdicts[ok] += 1
    assert verdicts[True] >= 50 and verdicts[False] >= 50, verdicts
