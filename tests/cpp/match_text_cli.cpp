// match_text_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of the assembly scan's routes over FASTA, track_text_cli with the
// match files in view:
//   match_text_cli --host|--device|--device-tracks [--chunk-bytes N] [--include-prefix LIST] [scan flags] -o DIR INPUT
//   match_text_cli --host|--device|--device-tracks ... -o DIR --each LIST
// --host is scanFastaToFiles, --device scanFastaToFilesDevice, --device-tracks scanFastaToFilesDevice with deviceTracks = true:
// the five window tracks and, under -m, the two match files formatted on the device (include/teloscope_mi355x_io.hpp).  All
// write DIR/<name>_*.bed / .bedgraph / _report.tsv and the console report + summary on stdout, so that a test can hold every
// byte of one route against another's.  --each LIST: one input path per line, every file through ONE Teloscope, file k's
// outputs under DIR/<k>.<file name>; a file that fails prints its error and the run goes on (exit status 1).
// At the end, on stderr:
//   match_text_stats <calls> <canonical lines> <non-canonical lines> <text bytes>      (ts_match_text_stats)
//   upload_stats <eight numbers>                                                       (ts_upload_stats)
//   route timing: read <ms> scan <ms> write <ms>, bases read back <bytes>               (ScanFastaTimes, summed over the inputs)
// -j is accepted and ignored.  Errors go to stderr as "Error: <message>" with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_filter.hpp"
#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

namespace {

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

}  // namespace

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".", eachList;
    std::vector<std::string> rawPatterns;
    std::vector<int> devices;
    bool hasPatterns = false, manualCuration = false;
    int route = -1;                                              // 2 device with device-formatted tracks, 1 device, 0 host
    size_t chunkBytes = size_t(256) << 20;
    uint64_t chunkLimit = 0xfffffffeull;
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string {
                if (i + 1 >= argc) throw UsageError("Option " + a + " is missing a required argument");
                return argv[++i];
            };
            if (a == "--device") route = 1;
            else if (a == "--device-tracks") route = 2;
            else if (a == "--host") route = 0;
            else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
            else if (a == "--chunk-limit") chunkLimit = std::stoull(val());
            else if (a == "--each") eachList = val();
            else if (a == "--include-prefix") addPrefixFilters(ui, val(), ui.includePrefixes, "--include-prefix");
            else if (a == "--devices") {
                std::istringstream ds(val());
                std::string d;
                while (std::getline(ds, d, ',')) if (!d.empty()) devices.push_back(std::stoi(d));
            }
            else if (a == "-f") input = val();
            else if (a == "-o") outDir = val();
            else if (a == "-j") (void)val();
            else if (a == "-c") canonical = val();
            else if (a == "-p") {
                hasPatterns = true;
                std::istringstream ps(val());
                std::string p;
                while (std::getline(ps, p, ',')) if (!p.empty()) rawPatterns.push_back(p);
            }
            else if (a == "-w") ui.windowSize = std::stoi(val());
            else if (a == "-s") ui.step = std::stoi(val());
            else if (a == "-t") ui.terminalLimit = std::stoi(val());
            else if (a == "-k") ui.maxMatchDist = static_cast<unsigned short>(std::stoi(val()));
            else if (a == "-d") ui.maxBlockDist = static_cast<unsigned short>(std::stoi(val()));
            else if (a == "-l") { ui.minBlockLen = static_cast<unsigned short>(std::stoi(val())); ui.minBlockLenSet = true; }
            else if (a == "-y") ui.minBlockDensity = std::stof(val());
            else if (a == "-x") ui.editDistance = static_cast<uint8_t>(std::stoi(val()));
            else if (a == "-r") { ui.outWinRepeats = true; ui.ultraFastMode = false; }
            else if (a == "-g") { ui.outGC = true; ui.ultraFastMode = false; }
            else if (a == "-e") { ui.outEntropy = true; ui.ultraFastMode = false; }
            else if (a == "-m") { ui.outMatches = true; ui.ultraFastMode = false; }
            else if (a == "-i") { ui.outITS = true; ui.ultraFastMode = false; }
            else if (a == "-a") ui.ultraFastMode = false;
            else if (a == "-u") ui.ultraFastMode = !(ui.outWinRepeats || ui.outGC || ui.outEntropy || ui.outITS || ui.outMatches);
            else if (a == "-n") manualCuration = true;
            else if (!a.empty() && a[0] != '-' && input.empty()) input = a;
            else throw UsageError("unknown option " + a);
        }
        if (route < 0) throw UsageError("one of --host, --device or --device-tracks is required");
        std::vector<std::string> inputs;
        if (!eachList.empty()) {
            std::ifstream in(eachList);
            if (!in) throw UsageError("cannot open the list " + eachList);
            for (std::string line; std::getline(in, line);) if (!line.empty()) inputs.push_back(line);
        } else if (!input.empty()) inputs.push_back(input);
        if (inputs.empty()) throw UsageError("No input file provided.");
        if (ui.step > ui.windowSize) throw UsageError("Step size cannot be larger than window size.");
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        std::filesystem::create_directories(outDir);
        const SequenceSelector selector(ui);
        Teloscope teloscope(ui, devices);
        int status = 0;
        ScanFastaTimes total;
        for (size_t k = 0; k < inputs.size(); ++k) {
            const std::string name = std::filesystem::path(inputs[k]).filename().string();
            const std::string outBase = outDir + "/" + (eachList.empty() ? name : std::to_string(k) + "." + name);
            try {
                ScanFastaTimes T;
                AssemblySummary summary;
                if (route >= 1) {
                    summary = scanFastaToFilesDevice(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes, &T, chunkLimit, route == 2,
                                                     &selector, std::cerr);
                } else {
                    FastaGroupReader reader(inputs[k], chunkBytes, size_t(4) << 20, true, selector.active());
                    SequenceSelection sel;
                    if (selector.active()) {
                        sel = selector.select(reader.primaryIds(), "paths");
                        reader.keep(sel.keep);
                        std::cerr << selectionMessage(sel) << "\n";
                    }
                    summary = scanFastaToFiles(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes, &T, size_t(4) << 20, -1, &reader);
                    if (selector.active()) {                     // (the Teloscope was made before the selection was known)
                        summary.filterInputCount = sel.inputCount;
                        summary.filterSelectedCount = sel.selectedCount;
                    }
                }
                total.read_ms += T.read_ms; total.scan_ms += T.scan_ms; total.write_ms += T.write_ms; total.bases_read_back += T.bases_read_back;
                printSummary(std::cout, summary, ui.ultraFastMode, outBase + "_report.tsv");
            } catch (const std::exception &e) {
                if (eachList.empty()) throw;
                std::fflush(stdout);
                std::fprintf(stderr, "Error: %s: %s\n", name.c_str(), e.what());
                status = EXIT_FAILURE;
            }
        }
        std::fflush(stdout);
        const std::array<uint64_t, 4> ms = teloscope.matchTextStats();
        std::fprintf(stderr, "match_text_stats %llu %llu %llu %llu\n", (unsigned long long)ms[0], (unsigned long long)ms[1], (unsigned long long)ms[2],
                     (unsigned long long)ms[3]);
        uint64_t up[8] = {0};
        if (ts_upload_stats(teloscope.context(), up) != TS_OK) throw std::runtime_error(ts_last_error(teloscope.context()));
        std::fprintf(stderr, "upload_stats");
        for (uint64_t v : up) std::fprintf(stderr, " %llu", (unsigned long long)v);
        std::fprintf(stderr, "\nroute timing: read %.1f ms scan %.1f ms write %.1f ms, bases read back %llu bytes\n", total.read_ms, total.scan_ms,
                     total.write_ms, (unsigned long long)total.bases_read_back);
        return status;
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
