"""The assembly scan's device route with device-formatted window tracks (scanFastaToFilesDevice, deviceTracks = true) through
tests/cpp/track_text_cli.cpp: --device-tracks against --host of the same binary on the committed FASTAs — the same exit status,
byte-equal console and byte-equal output files, every one of them.  With -m the flag falls back to host formatting and the
outputs are equal all the same.  The formatter by itself: tests/test_gpu_track_text.py; the scan entry point:
tests/test_gpu_scan_tracks.py."""
import shlex
import subprocess

import pytest

from tests import tracktext as T
from tests.test_fasta_chunk_reference_cpu import INPUTS
from tests.test_gpu_fasta_device import files_of

pytestmark = pytest.mark.gpu

FLAG_SETS = ["-r", "-g -e", "-r -g -e", "-r -g -e -i", "-u", "-r -g -e -m"]


@pytest.fixture(scope="module")
def tcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return T.build_track_cli(tmp_path_factory.mktemp("cpp") / "track_text_cli")


def run(tcli, out, route, flags, extra=()):
    lst = out.parent / (out.name + ".list")
    lst.write_text("".join(str(p) + "\n" for p in INPUTS))
    r = subprocess.run([tcli, route, "-o", str(out)] + shlex.split(flags) + list(extra) + ["--each", str(lst)], stdin=subprocess.DEVNULL,
                       capture_output=True, timeout=300)
    return r, files_of(out)


@pytest.fixture(scope="module")
def host_runs(tcli, tmp_path_factory):
    """the --host run of every flag set, made once"""
    memo = {}

    def get(flags):
        if flags not in memo:
            memo[flags] = run(tcli, tmp_path_factory.mktemp("host") / "out", "--host", flags)
        return memo[flags]
    return get


def same(d, dfiles, h, hfiles):
    assert d.returncode == h.returncode == 0, (d.returncode, h.returncode, d.stderr[-400:], h.stderr[-400:])
    assert d.stdout == h.stdout
    assert sorted(dfiles) == sorted(hfiles)
    for name in hfiles:
        assert dfiles[name] == hfiles[name], name


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_device_tracks_equal_the_host_route(tcli, host_runs, tmp_path, flags):
    assert len(INPUTS) >= 30
    h, hfiles = host_runs(flags)
    d, dfiles = run(tcli, tmp_path / "dev", "--device-tracks", flags)
    same(d, dfiles, h, hfiles)
    tracks = [f for f in dfiles if f.endswith(".bedgraph")]
    n_tracks = {"-r": 3, "-g -e": 2, "-u": 0}.get(flags, 5)
    assert len(tracks) == n_tracks * len(INPUTS)
    if n_tracks:
        assert sum(dfiles[f].count(b"\n") for f in tracks) > 100 * n_tracks
        assert any(b"windows" in dfiles[f] for f in dfiles if f.endswith("_report.tsv"))


def test_a_file_across_several_chunks(tcli, host_runs, tmp_path):
    """4 KiB chunks: every larger FASTA spans several, and every chunk's text is appended to the same track files."""
    flags = "-r -g -e"
    h, hfiles = host_runs(flags)
    d, dfiles = run(tcli, tmp_path / "dev", "--device-tracks", flags, ["--chunk-bytes", "4096"])
    same(d, dfiles, h, hfiles)
