"""FASTQ out of the BAM and SAM subsets through the routes of include/teloscope_mi355x_io.hpp (tests/cpp/read_fastq_out_cli.cpp):
the device routes' bytes == the host routes' of the same binary == the plain-Python rule (tests/readfastq.py) over the reads the CPU
oracle keeps, on a tiled set and mixed_5_6 written as BAM and as SAM with mixed FLAGs, on 1, 2 and 3 contexts, at two chunk sizes,
with both BAM walks, restored and --stored; the block report beside it equals the native subset's; a bad record gives the same
message and the same bytes before it; and ts_read_fastq_text_stats shows that the device formatted every kept record."""
import os
import random
import re
import subprocess

import pytest

from tests import readblocks as B
from tests import readfastq as Q
from tests import readsets as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED = "-l 42"
FLAGS = [TILED, R.SETS[0]]
IDS = ["tiled", R.SET_IDS[0]]
BAM_FLAGS = [0, 16, 4, 20, 0x900, 0x910, 83, 99]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from teloscope_amd import _capi
    _capi.lib()
    exe = tmp_path_factory.mktemp("read_fastq_out_cli") / "read_fastq_out_cli"
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "read_fastq_out_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(exe)])
    return str(exe)


def records_of(flags, kind, repeat=1):
    """The set's reads with bases as BAM records or SAM lines, FLAGs, names and QUALs mixed -> (the records, the reads)"""
    rng = random.Random(21)
    reads = [r for r in R.reads_for(flags) if r] * repeat
    out = []
    for i, r in enumerate(reads):
        flag = BAM_FLAGS[i % len(BAM_FLAGS)]
        name = b"" if i % 11 == 5 else b"read/%d:x" % i
        missing = i % 7 == 3
        if kind == "bam":
            out.append(Q.bam_record(name, flag, Q.bam_codes(r), None if missing else [rng.choice([0, 1, 20, 40, 92, 93, 94, 200]) for _ in r], n_cigar=i % 3))
        else:
            seq = bytes(c | 32 if (i + j) % 13 == 0 else c for j, c in enumerate(r))              # some lower case
            out.append(Q.sam_line(name, b"%d" % flag, seq, b"*" if missing else bytes(rng.randrange(33, 127) for _ in r),
                                  tags=[None, b"NM:i:0", b""][i % 3], eol=b"\r\n" if i % 5 == 2 else b"\n"))
    return out, reads


def file_of(kind, records):
    return B.bgzf(Q.bam_header() + b"".join(records), 3000) if kind == "bam" else b"@HD\tVN:1.6\n@CO\tc\n" + b"".join(records)


def expected(kind, records, passes, flags):
    return b"".join((Q.bam_text if kind == "bam" else Q.sam_text)(r, flags) for r, p in zip(records, passes) if p)


def run(cli, kind, path, flags, extra, each=False):
    args = [cli, "--" + kind, "--reads-per-batch", "37"] + extra + flags.split()
    if each:
        listing = str(path) + ".list"
        open(listing, "w").write(str(path) + "\n")
        for suffix in (".out", ".ok", ".err", ".partial", ".blocks"):
            if os.path.exists(str(path) + suffix):
                os.remove(str(path) + suffix)
        args += ["--each", listing]
    else:
        args.append(str(path))
    p = subprocess.run(args, stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    return p


DEVICE_RUNS = [["--contexts", "1", "--chunk-bytes", "4096", "--bam-walk", "serial"],
               ["--contexts", "2", "--chunk-bytes", "65536", "--bam-walk", "index"],
               ["--contexts", "3", "--chunk-bytes", "4096", "--bam-walk", "index"]]
STORED_RUN = ["--stored", "--contexts", "2", "--chunk-bytes", "4096", "--bam-walk", "serial"]


@pytest.mark.parametrize("kind", ["bam", "sam"])
@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
def test_device_equals_host_equals_the_rule(cli, tmp_path, flags, kind):
    records, reads = records_of(flags, kind)
    passes = [p for p, r in zip(R.oracle_passes(flags), R.reads_for(flags)) if r]
    assert len(passes) == len(records) and 0 < sum(passes) < len(passes)
    path = tmp_path / ("in." + kind)
    path.write_bytes(file_of(kind, records))
    restored, stored = expected(kind, records, passes, Q.RESTORE_STRAND), expected(kind, records, passes, 0)
    assert restored != stored and len(restored) == len(stored)
    ok = "read subset: kept %d of %d records, 0 block lines.\n" % (sum(passes), len(records))
    for extra, exp in [(["--host"], restored), (["--host", "--stored"], stored), (["--device"] + STORED_RUN, stored)] + \
                      [(["--device"] + r, restored) for r in DEVICE_RUNS]:
        p = run(cli, kind, path, flags, extra + ["--stats"])
        assert p.returncode == 0, (extra, p.stderr[-2000:])
        assert p.stdout == exp, extra
        err = p.stderr.decode()
        assert ok in err, (extra, err)
        m = re.search(r"read fastq text: (\d+) calls, (\d+) records, (\d+) bytes", err)
        if "--device" in extra:                                      # the device formatted every kept record, the host route none
            assert m and int(m.group(1)) > 0 and int(m.group(2)) == sum(passes) and int(m.group(3)) == len(exp), (extra, err)
        else:
            assert m and [int(x) for x in m.groups()] == [0, 0, 0], (extra, err)


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_block_report_beside_it_is_the_native_subsets(cli, tmp_path, kind):
    records, reads = records_of(TILED, kind)
    path = tmp_path / ("in." + kind)
    path.write_bytes(file_of(kind, records))
    names = [(Q.bam_text if kind == "bam" else Q.sam_text)(r, 0).split(b"\n", 1)[0][1:] for r in records]
    exp, kept = B.ref_report(list(zip(names, reads)), B.read_oracle(TILED))        # stored-SEQ coordinates, whatever the text's strand
    assert exp
    reports = {}
    for label, extra in [("native", ["--native", "--device", "--contexts", "2"]), ("host", ["--host"]),
                         ("device", ["--device", "--contexts", "2", "--chunk-bytes", "65536"]), ("stored", ["--device", "--stored"])]:
        blocks = tmp_path / (label + ".bed")
        p = run(cli, kind, path, TILED, extra + ["--blocks", str(blocks)])
        assert p.returncode == 0, (label, p.stderr[-2000:])
        reports[label] = blocks.read_bytes()
        assert ("%d block lines." % exp.count(b"\n")).encode() in p.stderr
    assert reports["native"] == exp
    assert reports["host"] == reports["device"] == reports["stored"] == reports["native"]


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_a_bad_record_gives_the_same_message_and_the_same_bytes_before_it(cli, tmp_path, kind):
    """The input holds several chunks; the bad record lies in the last.  Host and device routes throw the same text after the
    same bytes, on one context and on two."""
    records, reads = records_of(TILED, kind, repeat=5 if kind == "bam" else 1)
    at = len(records) - 9
    if kind == "bam":
        bad = bytearray(records[at])
        bad[0:4] = (7).to_bytes(4, "little")
        message = "invalid BAM record block_size"
    else:
        bad = b"bad\t16\t*\n"
        message = "SAM line %d: fewer than 11 fields" % (2 + at + 1)
    path = tmp_path / ("bad." + kind)
    path.write_bytes(file_of(kind, records[:at] + [bytes(bad)] + records[at:]))
    chunk = ["--chunk-bytes", str(1 << 20 if kind == "bam" else 65536)]
    got = {}
    for label, extra in [("host", ["--host"]), ("one", ["--device", "--contexts", "1"]), ("two", ["--device", "--contexts", "2"])]:
        p = run(cli, kind, path, TILED, extra + chunk, each=True)
        assert p.returncode == 0, (label, p.stderr[-2000:])
        assert os.path.exists(str(path) + ".err") and not os.path.exists(str(path) + ".ok"), label
        got[label] = (open(str(path) + ".err").read(), open(str(path) + ".partial", "rb").read())
    assert got["host"][0] == message + "\n"
    assert got["one"] == got["host"] and got["two"] == got["host"]
    partial = got["host"][1]
    assert partial and partial.count(b"\n") % 4 == 0
    passes = [p for p, r in zip(R.oracle_passes(TILED), R.reads_for(TILED)) if r] * (5 if kind == "bam" else 1)
    whole = expected(kind, records[:at], passes[:at], Q.RESTORE_STRAND)
    assert whole.startswith(partial)
