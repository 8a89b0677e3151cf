// fasta_device_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of the two routes of the assembly scan over FASTA,
//   fasta_device_cli --device|--host [--chunk-bytes N] [--chunk-limit N] [--devices LIST] [scan flags] -o DIR INPUT
//   fasta_device_cli --device|--host ... -o DIR --each LIST
//   fasta_device_cli --dump-records INPUT
// --host is scanFastaToFiles, --device scanFastaToFilesDevice (include/teloscope_mi355x_io.hpp); both write DIR/<name>_*.bed /
// .bedgraph / _report.tsv and the console report + summary on stdout, so that a test can hold every byte of one route against
// the other's.  --each LIST: LIST is a text file with one input path per line; every file goes through ONE Teloscope in one
// process, file k's outputs under DIR/<k>.<file name>; a file that fails prints its error and the run goes on (exit status 1).
// --chunk-bytes is the device route's chunk (the host route's group), --chunk-limit the most a device chunk may grow to,
// --devices the HIP ordinals the Teloscope is made over (an ordinal may repeat).
// --dump-records INPUT touches no device: the host reader's view of the file (FastaGroupReader, joined lines, as scanFastaToFiles
// reads it), one line per record: name <TAB> bases <TAB> FNV-1a 64 of the bases (hex) <TAB> runs as S:start:len / G:start:len.
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

void dumpRecord(const std::string &name, const char *bases, size_t n, const PathComponents &pc) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= static_cast<unsigned char>(bases[i]); h *= 0x100000001b3ull; }
    std::printf("%s\t%zu\t%016llx\t", name.c_str(), n, static_cast<unsigned long long>(h));
    size_t si = 0, gi = 0;
    bool firstRun = true;
    while (si < pc.segments.size() || gi < pc.gaps.size()) {
        const bool seg = gi >= pc.gaps.size() || (si < pc.segments.size() && pc.segments[si].first < pc.gaps[gi].start);
        if (!firstRun) std::printf(",");
        firstRun = false;
        if (seg) { std::printf("S:%llu:%llu", static_cast<unsigned long long>(pc.segments[si].first), static_cast<unsigned long long>(pc.segments[si].second)); ++si; }
        else { std::printf("G:%llu:%u", static_cast<unsigned long long>(pc.gaps[gi].start), pc.gaps[gi].length); ++gi; }
    }
    std::printf("\n");
}

int dumpRecords(const std::string &file) {
    FastaGroupReader reader(file, size_t(256) << 20, size_t(4) << 20, false, false);
    detail::FastaGroup g;
    while (reader.next(g)) {
        for (size_t r = 0; r < g.records.size(); ++r) dumpRecord(g.records[r].header, g.records[r].data.get(), g.records[r].size, g.comps[r]);
        for (const FastaRecord &r : g.owned) dumpRecord(r.header, r.sequence.data(), r.sequence.size(), splitPath(r.sequence));
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".", eachList, dumpFile;
    std::vector<std::string> rawPatterns;
    std::vector<int> devices;
    bool hasPatterns = false, manualCuration = false;
    int route = -1;                                              // 1 device, 0 host
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
            else if (a == "--host") route = 0;
            else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
            else if (a == "--chunk-limit") chunkLimit = std::stoull(val());
            else if (a == "--each") eachList = val();
            else if (a == "--dump-records") dumpFile = val();
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
        if (!dumpFile.empty()) return dumpRecords(dumpFile);
        if (route < 0) throw UsageError("one of --device, --host or --dump-records is required");
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
                const AssemblySummary summary = route == 1
                    ? scanFastaToFilesDevice(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes, nullptr, chunkLimit)
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
