// track_text_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of the assembly scan's routes over FASTA with the flags of
// fasta_device_cli,
//   track_text_cli --host|--device|--device-tracks [--chunk-bytes N] [--chunk-limit N] [--devices LIST] [scan flags] -o DIR INPUT
//   track_text_cli --host|--device|--device-tracks ... -o DIR --each LIST
//   track_text_cli --check-put
// --host is scanFastaToFiles, --device scanFastaToFilesDevice, --device-tracks scanFastaToFilesDevice with deviceTracks = true:
// the five window tracks formatted on the device (include/teloscope_mi355x_io.hpp).  All write DIR/<name>_*.bed / .bedgraph /
// _report.tsv and the console report + summary on stdout, so that a test can hold every byte of one route against another's.
// --each LIST: one input path per line, every file through ONE Teloscope, file k's outputs under DIR/<k>.<file name>; a file that
// fails prints its error and the run goes on (exit status 1).
// --check-put touches no device: detail::put(float) — the host writers' memoised to_chars — against operator<<(float) for every
// n / d with d <= 2048, every GC value of windows of up to 2048 bases, k / 1000 for k <= 2000 and -1; prints "ok <n> values".
// -j is accepted and ignored.  Errors go to stderr as "Error: <message>" with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

namespace {

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

uint64_t checked = 0;

void checkOne(float v) {
    std::string got;
    detail::put(got, v);
    detail::put(got, v);                                         // (the second time out of the memo)
    std::ostringstream want;
    want << v << v;
    if (got != want.str()) {
        char what[96];
        std::snprintf(what, sizeof what, "%.9g: put \"%s\" stream \"%s\"", static_cast<double>(v), got.c_str(), want.str().c_str());
        throw std::runtime_error(what);
    }
    ++checked;
}

int checkPut() {
    for (uint32_t d = 1; d <= 2048; ++d)
        for (uint32_t n = 0; n <= d; ++n) {
            checkOne(static_cast<float>(n) / d);
            const uint32_t counts[4] = {0, n, 0, 0};
            checkOne(ts_gc_content(counts, d));
        }
    for (uint32_t k = 0; k <= 2000; ++k) checkOne(static_cast<float>(k) / 1000.0f);
    checkOne(-1.0f);
    std::printf("ok %llu values\n", static_cast<unsigned long long>(checked));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".", eachList;
    std::vector<std::string> rawPatterns;
    std::vector<int> devices;
    bool hasPatterns = false, manualCuration = false;
    int route = -1;                                              // 2 device with device-formatted tracks, 1 device, 0 host
    bool checkPutOnly = false;
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
            else if (a == "--check-put") checkPutOnly = true;
            else if (a == "--host") route = 0;
            else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
            else if (a == "--chunk-limit") chunkLimit = std::stoull(val());
            else if (a == "--each") eachList = val();
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
        if (checkPutOnly) return checkPut();
        if (route < 0) throw UsageError("one of --host, --device, --device-tracks or --check-put is required");
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
        Teloscope teloscope(ui, devices);
        int status = 0;
        for (size_t k = 0; k < inputs.size(); ++k) {
            const std::string name = std::filesystem::path(inputs[k]).filename().string();
            const std::string outBase = outDir + "/" + (eachList.empty() ? name : std::to_string(k) + "." + name);
            try {
                const AssemblySummary summary = route >= 1
                    ? scanFastaToFilesDevice(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes, nullptr, chunkLimit, route == 2)
                    : scanFastaToFiles(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes);
                printSummary(std::cout, summary, ui.ultraFastMode, outBase + "_report.tsv");
            } catch (const std::exception &e) {
                if (eachList.empty()) throw;
                std::fflush(stdout);
                std::fprintf(stderr, "Error: %s: %s\n", name.c_str(), e.what());
                status = EXIT_FAILURE;
            }
        }
        return status;
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
