"""The assembly device routes on a Teloscope of several contexts, as far as they can be checked without a GPU: the test program
tests/cpp/assembly_routes_multi_cli.cpp builds against include/ and libteloscan with warnings as errors and names its options,
and the headers declare what tests/test_gpu_assembly_routes_multi.py drives."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cli(out):
    libdir = os.path.join(ROOT, "teloscope_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "assembly_routes_multi_cli.cpp"), "-L", libdir, "-lteloscan",
                           "-Wl,-rpath," + libdir, "-pthread", "-lz", "-o", str(out)])
    return str(out)


def test_cli_builds_and_names_its_options(tmp_path):
    """Fails without the feature: the program passes perDevice to both entry points."""
    import teloscope_amd  # noqa: F401  (makes sure libteloscan.so is built)
    cli = build_cli(tmp_path / "assembly_routes_multi_cli")
    r = subprocess.run([cli, "--help"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == ""
    for option in ("--fasta", "--gfa", "--device", "--host", "--devices", "--chunk-bytes", "--device-tracks", "--chunk-limit", "--each",
                   "--include-bed", "--exclude-bed", "--include-prefix", "--exclude-prefix", "-o"):
        assert option in r.stdout, option
    r = subprocess.run([cli, "--fasta"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("Error: one of --device and --host is required")
    r = subprocess.run([cli, "--device", "--gfa"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("Error: No input file provided.")


DECLARATIONS = r"""
#include <type_traits>
#include "teloscope_mi355x_filter.hpp"
#include "teloscope_mi355x_gfa.hpp"
#include "teloscope_mi355x_io.hpp"
using namespace teloscope_mi355x;
using PerDevice = std::vector<AssemblyRouteDeviceStats>;

template <class T, class F> constexpr bool is(F AssemblyRouteDeviceStats::*) { return std::is_same<T, F>::value; }
static_assert(is<int>(&AssemblyRouteDeviceStats::device), "device ordinal");
static_assert(is<uint64_t>(&AssemblyRouteDeviceStats::chunks) && is<uint64_t>(&AssemblyRouteDeviceStats::records) &&
              is<uint64_t>(&AssemblyRouteDeviceStats::basesScanned) && is<uint64_t>(&AssemblyRouteDeviceStats::bytesReceived), "counts");
static_assert(is<double>(&AssemblyRouteDeviceStats::msFill) && is<double>(&AssemblyRouteDeviceStats::msStage) &&
              is<double>(&AssemblyRouteDeviceStats::msFrameWait) && is<double>(&AssemblyRouteDeviceStats::msCommit) &&
              is<double>(&AssemblyRouteDeviceStats::msIndex) && is<double>(&AssemblyRouteDeviceStats::msJoin) &&
              is<double>(&AssemblyRouteDeviceStats::msScan), "milliseconds");
static_assert(TELOSCAN_ABI_VERSION == 4, "no new entry point: the ABI stays");

// perDevice is the trailing argument of both entry points, and may be left out
AssemblySummary fasta(Teloscope &t, const SequenceSelector &sel, PerDevice *per) {
    scanFastaToFilesDevice(t, "in", "out", std::cout);
    return scanFastaToFilesDevice(t, "in", "out", std::cout, false, 64, nullptr, 64, false, &sel, std::cerr, 0, per);
}
GfaAnnotateStats gfa(Teloscope &t, const SequenceSelector &sel, PerDevice *per) {
    annotateGfaDevice(t, "in", "out");
    annotateGfaDevice(t, "in", "out", sel);
    annotateGfaDevice(t, "in", "out", std::cerr, 64, per);
    return annotateGfaDevice(t, "in", "out", sel, std::cerr, 64, per);
}
// every scan method and stats getter on a chosen context; the forms without one stay
void scans(Teloscope &t, const std::vector<Teloscope::Segment> &segs, const std::vector<const char *> &names,
           std::vector<ts_segment_counts> &counts, TrackText &text, const std::vector<RecordView> &records) {
    static_assert(std::is_same<decltype(t.context(1)), ts_ctx *>::value && std::is_same<decltype(t.context()), ts_ctx *>::value, "context(i)");
    t.scanSegments(segs);                              t.scanSegments(segs, false, 1);
    t.scanSegmentsNoMatches(segs, counts);             t.scanSegmentsNoMatches(segs, counts, 1);
    t.scanSegmentsTrackText(segs, names, counts, text); t.scanSegmentsTrackText(segs, names, counts, text, 1);
    t.scanSegmentsText(segs, names, counts, text);     t.scanSegmentsText(segs, names, counts, text, 1);
    t.terminalEnds(segs);                              t.terminalEnds(segs, 1);
    t.deviceInputStats();                              t.deviceInputStats(1);
    t.terminalEndsStats();                             t.terminalEndsStats(1);
    t.matchTextStats();                                t.matchTextStats(1);
    walkRecordViews(t, records);                       walkRecordViews(t, records, 0, nullptr, nullptr, &text, 1);
}
"""


def test_headers_declare_the_per_context_forms(tmp_path):
    """Fails without the feature: a translation unit that names AssemblyRouteDeviceStats' fields by type, passes perDevice to both
    entry points and calls every scan method and stats getter with and without a context compiles against include/."""
    unit = tmp_path / "declarations.cpp"
    unit.write_text(DECLARATIONS)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(unit)], stdin=subprocess.DEVNULL,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
