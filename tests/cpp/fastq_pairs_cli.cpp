// fastq_pairs_cli.cpp — TEST INFRASTRUCTURE: the read subset of interleaved paired FASTQ (include/teloscan.h: "Interleaved paired
// FASTQ") on a ReadTelomereFilter of one or several contexts, through the host route (fastqSubsetPaired) or the device route
// (fastqSubsetPairedDevice: pairs framed, names compared, reads judged and kept pairs gathered on the GPU), so that the two can be
// compared on the same input by the same binary.
// Usage: fastq_pairs_cli [--device|--host] [--contexts N] [--chunk-bytes N] [--reads-per-batch N] [--blocks]
//                        [-c -p -x -l -y -k -d -t ...] [file|-]          (no file: stdin)
//        --contexts N: N contexts on device 0 (the ring deals the chunks)
//        --blocks: the read block report beside the subset, to <file>.blocks (stdin: stdin.blocks)
//        fastq_pairs_cli ... --each LIST   every file named in LIST through one filter: <file>.out and <file>.ok (the statistics),
//                                          or <file>.err with the message and <file>.partial with what was written before it; a
//                                          line "<file" puts the file on descriptor 0 and runs the route on "-"
// stdout carries the subset.  stderr ends with "FASTQ paired subset: kept K of N records."; a failure is "Error: <message>" and
// exit status 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, each;
    bool device = true, withBlocks = false;
    size_t readsPerBatch = 1u << 20, chunkBytes = 0;
    int contexts = 1;
    std::vector<std::string> rawPatterns;
    bool hasPatterns = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) exit(EXIT_FAILURE); return argv[++i]; };
        auto list = [&](const std::string &v, auto &&item) {
            std::istringstream in(v);
            std::string x;
            while (std::getline(in, x, ',')) if (!x.empty()) item(x);
        };
        if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--each") each = val();
        else if (a == "--blocks") withBlocks = true;
        else if (a == "--contexts") contexts = std::max(1, std::stoi(val()));
        else if (a == "--reads-per-batch") readsPerBatch = static_cast<size_t>(std::stoull(val()));
        else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
        else if (a == "-c") canonical = val();
        else if (a == "-p") { hasPatterns = true; list(val(), [&](const std::string &x) { rawPatterns.push_back(x); }); }
        else if (a == "-j") (void)val();                        // (threads of the reference's host pool: nothing to set here)
        else if (a == "-t") ui.terminalLimit = std::stoi(val());
        else if (a == "-k") ui.maxMatchDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-d") ui.maxBlockDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-l") { ui.minBlockLen = static_cast<unsigned short>(std::stoi(val())); ui.minBlockLenSet = true; }
        else if (a == "-y") ui.minBlockDensity = std::stof(val());
        else if (a == "-x") ui.editDistance = static_cast<uint8_t>(std::stoi(val()));
        else if (!a.empty() && (a[0] != '-' || a == "-") && input.empty()) input = a;
    }
    if (input.empty()) input = "-";
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui, std::vector<int>(static_cast<size_t>(contexts), 0));      // (no device: throws — there is no host scan behind either route)
        filter.bindThreadToDevice();
        const size_t chunk = chunkBytes ? chunkBytes : size_t(256) << 20;
        auto subset = [&](const std::string &path, std::ostream &out, std::ostream *blocks) {
            return device ? fastqSubsetPairedDevice(path, out, filter, readsPerBatch, chunk, nullptr, blocks) : fastqSubsetPaired(path, out, filter, readsPerBatch, chunk, blocks);
        };
        auto figures = [](const FastqSubsetResult &s) {
            char line[200];
            snprintf(line, sizeof line, "FASTQ paired subset: kept %llu of %llu records.", (unsigned long long)s.kept, (unsigned long long)s.total);
            return std::string(line);
        };
        if (!each.empty()) {
            std::ifstream list(each);
            std::string path;
            while (std::getline(list, path)) {
                if (path.empty()) continue;
                const bool viaStdin = path[0] == '<';           // "<file": the file becomes descriptor 0 and the route reads "-"
                if (viaStdin) path.erase(0, 1);
                try {
                    if (viaStdin) {
                        const int fd = ::open(path.c_str(), O_RDONLY);
                        if (fd < 0 || ::dup2(fd, 0) < 0) throw std::runtime_error("cannot put '" + path + "' on stdin");
                        if (fd != 0) ::close(fd);
                    }
                    std::ofstream out(path + ".out", std::ios::binary), bed;
                    if (withBlocks) bed.open(path + ".blocks", std::ios::binary);
                    const FastqSubsetResult s = subset(viaStdin ? "-" : path, out, withBlocks ? &bed : nullptr);
                    out.close();
                    std::ofstream(path + ".ok") << figures(s) << "\n";
                } catch (const std::exception &e) {
                    std::rename((path + ".out").c_str(), (path + ".partial").c_str());     // (what was written before the failure)
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
            return 0;
        }
        std::ofstream bed;
        if (withBlocks) bed.open((input == "-" ? std::string("stdin") : input) + ".blocks", std::ios::binary);
        const FastqSubsetResult s = subset(input, std::cout, withBlocks ? &bed : nullptr);
        std::cout.flush();
        fprintf(stderr, "%s\n", figures(s).c_str());
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
