"""bench.py's command line without a GPU: --full and --dump-outputs are there, and --dump-outputs is refused where it has
nothing single-GPU to write (before any rank process, build or device is touched)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=120)


def test_help_names_full_and_dump_outputs():
    r = _bench("--help")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_dump_outputs_is_refused_with_more_than_one_gpu(tmp_path):
    r = _bench("--gpus", "2", "--dump-outputs", str(tmp_path / "out"))
    assert r.returncode == 2 and "--dump-outputs" in r.stderr and "--gpus 1" in r.stderr
    assert not (tmp_path / "out").exists()
