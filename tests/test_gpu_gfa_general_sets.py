"""The GFA annotation under a pattern set the tiled kernel does not take (-p TTAGGG,TTAGG): annotateGfa and annotateGfaDevice
both get their per-end lengths from ts_terminal_ends, which reduces such a set's records on the device.  Two committed graphs,
one with paths and one pathless, through tests/cpp/gfa_device_cli.cpp: --device against --host byte for byte (the comparison of
tests/test_gpu_gfa_device.py), and the telomere nodes of the written graph against the nodes the CPU oracle's per-side lengths
give (tests/harness.py: gfa_annotations).  This pins that the route of the lengths changed no file."""
import os

import pytest

from tests import harness as H
from tests.test_gfa_chunk_reference_cpu import build_cli
from tests.test_gfa_mode import parse_doc
from tests.test_gpu_gfa_device import both

pytestmark = pytest.mark.gpu

FLAGS = ["-p", "TTAGGG,TTAGG", "-l", "60"]
GRAPHS = ["gfa_path_orient_pairs_small.gfa", "gfa_pathless_small.gfa"]


@pytest.fixture(scope="module")
def dcli(tmp_path_factory):
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    return build_cli(tmp_path_factory.mktemp("cpp") / "gfa_device_cli")


@pytest.mark.parametrize("name", GRAPHS)
def test_both_routes_write_the_oracles_nodes_under_a_mixed_length_set(dcli, tmp_path, name):
    from tests.backends import OracleBackend
    path = H.golden_path("testFiles/" + name)
    _, paths = H.parse_gfa(path)
    assert bool(paths) == (name == GRAPHS[0])                       # one graph with paths, one pathless
    d, files = both(dcli, tmp_path, FLAGS, path)
    assert d.returncode == 0, d.stderr[-300:]
    out = tmp_path / "run--device" / (name + ".telo.annotated.gfa")
    assert os.path.relpath(str(out), str(tmp_path / "run--device")) in files
    opts = H.parse_cli("-f %s %s" % (path, " ".join(FLAGS)))
    want = H.gfa_annotations(OracleBackend(opts), opts, path)
    assert len(want) == 4
    got = {(n, int(t["TL"])) for n, t in parse_doc(str(out))["tel_segs"]}
    assert got == {(node, tl) for _, _, _, node, tl in want}
