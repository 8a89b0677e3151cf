"""The FASTA-text half of the packed upload on the host: ts::pack_text (teloscope_amd/csrc/pack.cpp: AVX2 / BMI2, 32 text bytes a
round, the line ends' slots taken out of the codes), the text walks strip_copy / text_locate / strip_take and the staging
workers' range cuts (teloscope_amd/csrc/text_core.h), compiled for the host by g++ under ASan + UBSan together with a program of
their own (tests/cpp/text_pack_host.cpp) and compared there with a statement of the same thing a byte at a time.  Every text and
every output buffer is a heap block of exactly the size the contract allows, so one byte too many in either direction is a
sanitizer report.  No GPU needed, nothing loaded into Python is under a sanitizer.

What the program pins beyond equality: pack_text writes exactly (taken + 3) / 4 bytes (the staging workers of one chunk write
adjacent bytes), strip_take writes no byte beyond the n it is asked for (the mixed block strips into the end of its 16384-byte
buffer), and neither leaves its cursor between a carriage return and its line feed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_CASES = 600


def fields(line):
    words = line.split()
    return {k: int(v) for k, v in zip(words[1::2], words[2::2])}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("text_pack")
    out = str(d / "text_pack_host")
    base = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            os.path.join(ROOT, "tests", "cpp", "text_pack_host.cpp"), os.path.join(ROOT, "teloscope_amd", "csrc", "pack.cpp"), "-o", out]
    for more in ([], ["-static-libasan"]):                         # (a preloaded library may keep a shared ASan runtime from starting)
        subprocess.check_call(base + more)
        r = subprocess.run([out], capture_output=True)
        if r.returncode == 2 and b"usage" in r.stderr:
            break
    assert r.returncode == 2 and b"usage" in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, timeout=1200, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    return r.stdout.decode()


def vector_paths_ran(out):
    """The AVX2 / BMI2 rounds are what most of this file is about; on a host without them the program has checked the scalar
    loops alone (it must still pass), and the test says so instead of passing for the wrong reason."""
    if not (out["avx2"] and out["bmi2"]):
        pytest.skip("the path under test did not run: this host has no AVX2 / BMI2, only the scalar loops were checked")


def test_every_short_text_over_base_invalid_cr_lf(exe):
    """All 22 369 621 texts of 12 bytes or fewer over {A, n, CR, LF}: pack_text in consecutive calls and entered at every base,
    strip_take, strip_copy and text_locate.  Texts of up to 6 bytes with every (first base, count) pair; longer ones with every
    count from the first base and every first base to the end — the family holds every suffix of each of its texts and none of
    the functions looks in front of its cursor, so the pairs left out are another text's.  (In parallel parts: one process
    would take minutes under the sanitizers.)"""
    parts = max(1, min(8, len(os.sched_getaffinity(0))))
    procs = [subprocess.Popen([exe, "exhaustive", "12", "0", "6", str(p), str(parts)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV)
             for p in range(parts)]
    texts = 0
    for p in procs:
        out, err = p.communicate(timeout=3000)
        assert p.returncode == 0 and not err, err.decode(errors="replace")[-3000:]
        out = fields(out.decode())
        texts += out["texts"]
        assert out["cursor_between_cr_and_lf_after_pack_text"] == 0
    assert texts == sum(4 ** n for n in range(13))


def test_every_short_text_across_the_end_of_a_vector_round(exe):
    """The same family up to 7 bytes, behind 27 bases and in front of 40: the texts lie in bytes 27 to 33, so every combination
    of line-end bytes meets bytes 30 to 33 of a 32-byte round (the carriage return in byte 31 whose fate byte 32 decides), and
    entering at every base moves the rounds over them."""
    out = fields(run([exe, "exhaustive", "7", "27", "0", "0", "1"]))
    assert out["texts"] == sum(4 ** n for n in range(8))
    assert out["cursor_between_cr_and_lf_after_pack_text"] == 0
    vector_paths_ran(out)


def test_rendered_random_sequences(exe):
    """Random sequences of up to 700 bases (and a few of 40 000 to 60 000, for calls of 16384 bases) over ACGT and ACGTacgtNnRY,
    folded and not, in lines of 1 to 80 bases ending in LF, CRLF or a mix, with lone carriage returns inside lines, CR CR LF,
    blank lines, and a text that ends in CR, CRLF, LF or a base.  The generator has to reach what the vector code decides on:
    a carriage return in byte 31 of a round with its line feed in byte 32, and an invalid run that goes on across a line end,
    each in at least a tenth of the cases."""
    out = fields(run([exe, "random", "20261018", str(RANDOM_CASES)]))
    print(out)
    assert out["cases"] == RANDOM_CASES
    assert 10 * out["cr_in_byte_31_lf_in_byte_32"] >= RANDOM_CASES
    assert 10 * out["invalid_run_across_line_end"] >= RANDOM_CASES
    assert out["cursor_between_cr_and_lf_after_pack_text"] == 0
    vector_paths_ran(out)


def test_python_statement_of_text_to_bases():
    """tests/textpieces.py: the replace-based to_bases that the GPU tests use for long texts against the rule stated a byte at a
    time — on every text of 8 bytes or fewer over {A, n, CR, LF} and on rendered sequences of every width and style."""
    import itertools

    import numpy as np

    from tests import textpieces as T
    for n in range(9):
        for t in itertools.product(b"An\r\n", repeat=n):
            assert T.to_bases(bytes(t)) == T.to_bases_bytewise(bytes(t)), bytes(t)
    rng = np.random.default_rng(3)
    for i, width in enumerate(T.WIDTHS):
        for style in T.STYLES:
            seq = bytes(b"ACGTNacgtnRY"[int(x)] for x in rng.integers(0, 12, size=int(rng.integers(1, 900))))
            text = T.render(seq, width, style, rng, first=(30 + i % 4) if i % 2 else None)
            assert T.to_bases(text) == T.to_bases_bytewise(text)
            assert style == "extras" or T.to_bases(text) == seq


def test_range_cuts(exe):
    """The staging workers' ranges for chunks of 1 to 2^27 positions, 1 to 8 workers, without pieces, with plain pieces, with
    text pieces and with both: from 0 to P, never descending, every cut in front of P a multiple of 4 (a range's first code
    begins a byte; a cut AT P leaves the workers behind it nothing, and P is any number), and a cut that is not a multiple of
    4096 is the start of a text piece rounded up to 4."""
    out = fields(run([exe, "cuts", "7", "900"]))
    assert out["checked"] >= 900 * 4 * 8 and out["cuts_at_a_text_piece"] > 1000


def test_upload_stats_in_header_library_and_binding():
    """ts_upload_stats: declared, exported, bound with its argument types, refuses null arguments, and counts nothing on a
    context that has uploaded nothing."""
    import re

    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd.cli import parse_cli, user_input
    hdr = open(os.path.join(ROOT, "include", "teloscan.h")).read()
    assert re.search(r"int\s+ts_upload_stats\(const ts_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    assert "ts_upload_stats" in K.SYMBOLS and K.lib().ts_upload_stats.argtypes is not None
    assert K.lib().ts_upload_stats(None, None) == K.TS_ERR_INVALID_ARG
    tel = ta.Teloscope(user_input(parse_cli("x.fa -r"), device=K.DEVICE_NONE))
    assert tel.upload_stats() == (0,) * 8
