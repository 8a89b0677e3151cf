// fastq_device_cli.cpp — TEST INFRASTRUCTURE: --fastq-subset through either route of include/teloscope_mi355x_io.hpp, the host
// one (fastqSubset: lines found and sequences copied on the host) or the device one (fastqSubsetDevice: lines indexed, records
// framed, sequences staged and passing records gathered on the GPU), so that the two can be compared on the same input by the
// same binary.
// Usage: fastq_device_cli --fastq-subset [--device|--host] [--fastq-chunk-bytes N] [--reads-per-batch N]
//                         [-c -p -x -l -y -k -d -t ...] [file|-]          (no file: stdin)
//        fastq_device_cli --fastq-subset-each LIST ...   every file named in LIST through one filter: <file>.out and <file>.ok,
//                                                        or <file>.err with the message (the convention of manifest_cli)
// stderr carries the reference's line ("FASTQ subset: kept %d of %d reads.").
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, fastqList;
    bool fastqSubsetMode = false, device = true;
    size_t readsPerBatch = 1u << 20, chunkBytes = 0;
    std::vector<std::string> rawPatterns;
    bool hasPatterns = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) exit(EXIT_FAILURE); return argv[++i]; };
        if (a == "--fastq-subset") fastqSubsetMode = true;
        else if (a == "--fastq-subset-each") { fastqSubsetMode = true; fastqList = val(); }
        else if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--reads-per-batch") readsPerBatch = static_cast<size_t>(std::stoull(val()));
        else if (a == "--fastq-chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
        else if (a == "-f") input = val();
        else if (a == "-c") canonical = val();
        else if (a == "-p") {
            hasPatterns = true;
            std::istringstream ps(val());
            std::string p;
            while (std::getline(ps, p, ',')) if (!p.empty()) rawPatterns.push_back(p);
        }
        else if (a == "-j") (void)val();                        // (threads of the reference's host pool: nothing to set here)
        else if (a == "-t") ui.terminalLimit = std::stoi(val());
        else if (a == "-k") ui.maxMatchDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-d") ui.maxBlockDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-l") { ui.minBlockLen = static_cast<unsigned short>(std::stoi(val())); ui.minBlockLenSet = true; }
        else if (a == "-y") ui.minBlockDensity = std::stof(val());
        else if (a == "-x") ui.editDistance = static_cast<uint8_t>(std::stoi(val()));
        else if (!a.empty() && (a[0] != '-' || a == "-") && input.empty()) input = a;
    }
    if (!fastqSubsetMode) { fprintf(stderr, "fastq_device_cli: --fastq-subset or --fastq-subset-each is required\n"); return EXIT_FAILURE; }
    auto subset = [&](const std::string &path, std::ostream &out, ReadTelomereFilter &filter) {
        if (device) return chunkBytes ? fastqSubsetDevice(path, out, filter, readsPerBatch, chunkBytes) : fastqSubsetDevice(path, out, filter, readsPerBatch);
        return chunkBytes ? fastqSubset(path, out, filter, readsPerBatch, chunkBytes) : fastqSubset(path, out, filter, readsPerBatch);
    };
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui);                          // (no device: throws — there is no host scan behind either route)
        filter.bindThreadToDevice();
        if (!fastqList.empty()) {
            std::ifstream list(fastqList);
            std::string path;
            while (std::getline(list, path)) {
                if (path.empty()) continue;
                try {
                    std::ofstream out(path + ".out", std::ios::binary);
                    const FastqSubsetResult r = subset(path, out, filter);
                    out.close();
                    std::ofstream(path + ".ok") << r.kept << " " << r.total << "\n";
                } catch (const std::exception &e) {
                    std::remove((path + ".out").c_str());
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
            return 0;
        }
        const FastqSubsetResult r = subset(input.empty() ? "-" : input, std::cout, filter);
        fprintf(stderr, "FASTQ subset: kept %llu of %llu reads.\n", (unsigned long long)r.kept, (unsigned long long)r.total);
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
