// read_fastq_out_cli.cpp — TEST INFRASTRUCTURE: the BAM and SAM subsets of include/teloscope_mi355x_io.hpp with FASTQ out
// (bamSubsetFastq, samSubsetFastq and their device forms), on a ReadTelomereFilter of one or several contexts, so that host and
// device routes can be compared on the same input by the same binary.
// Usage: read_fastq_out_cli --bam|--sam [--host|--device] [--stored] [--native] [--blocks FILE] [--contexts N] [--chunk-bytes N]
//                           [--reads-per-batch N] [--bam-walk serial|index] [--stats] [-c -p -x -l -y -k -d -t ...] [file|-]
//        read_fastq_out_cli ... --each LIST   every file named in LIST through one filter: <file>.out and <file>.ok (the
//                                             statistics), or <file>.err with the message and <file>.partial with what was written
//                                             before it; with --blocks (its FILE is not used then) the report goes to <file>.blocks
// --stored writes SEQ and QUAL as stored (ReadFastqOutput::restoreStrand = false); --native writes the subset in the input's own
// format (bamSubset / samSubset and their device forms), for comparisons.  stdout carries the output.  stderr ends with
// "read subset: kept K of T records, B block lines."; --stats adds "read fastq text: C calls, R records, B bytes"
// (ts_read_fastq_text_stats, summed over the contexts).  A failure is "Error: <message>" and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, each, blocksPath, mode;
    bool device = true, wantBlocks = false, wantStats = false, native = false;
    ReadFastqOutput fastq;
    size_t readsPerBatch = 1u << 20, chunkBytes = 0, contexts = 1;
    BamRecordWalk walk = BamRecordWalk::Index;
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
        if (a == "--bam" || a == "--sam") mode = a;
        else if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--stored") fastq.restoreStrand = false;
        else if (a == "--native") native = true;
        else if (a == "--blocks") { blocksPath = val(); wantBlocks = true; }
        else if (a == "--stats") wantStats = true;
        else if (a == "--each") each = val();
        else if (a == "--contexts") contexts = static_cast<size_t>(std::stoull(val()));
        else if (a == "--reads-per-batch") readsPerBatch = static_cast<size_t>(std::stoull(val()));
        else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
        else if (a == "--bam-walk") walk = val() == "serial" ? BamRecordWalk::Serial : BamRecordWalk::Index;
        else if (a == "-c") canonical = val();
        else if (a == "-p") { hasPatterns = true; list(val(), [&](const std::string &x) { rawPatterns.push_back(x); }); }
        else if (a == "-j") (void)val();
        else if (a == "-t") ui.terminalLimit = std::stoi(val());
        else if (a == "-k") ui.maxMatchDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-d") ui.maxBlockDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-l") { ui.minBlockLen = static_cast<unsigned short>(std::stoi(val())); ui.minBlockLenSet = true; }
        else if (a == "-y") ui.minBlockDensity = std::stof(val());
        else if (a == "-x") ui.editDistance = static_cast<uint8_t>(std::stoi(val()));
        else if (!a.empty() && (a[0] != '-' || a == "-") && input.empty()) input = a;
    }
    if (mode.empty()) { fprintf(stderr, "read_fastq_out_cli: --bam or --sam is required\n"); return EXIT_FAILURE; }
    if (input.empty()) input = "-";
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui, std::vector<int>(std::max<size_t>(contexts, 1), 0));     // (no device: throws — neither route scans on the host)
        filter.bindThreadToDevice();
        const size_t chunk = chunkBytes ? chunkBytes : size_t(256) << 20;
        struct Figures { uint64_t kept, total, blockLines; };
        auto subset = [&](const std::string &path, std::ostream &out, std::ostream *blocks) -> Figures {
            if (mode == "--sam") {
                const SamSubsetStats s = native ? (device ? samSubsetDevice(path, out, filter, readsPerBatch, chunk, nullptr, blocks)
                                                          : samSubset(path, out, filter, readsPerBatch, chunk, blocks))
                                                : (device ? samSubsetFastqDevice(path, out, filter, fastq, readsPerBatch, chunk, nullptr, blocks)
                                                          : samSubsetFastq(path, out, filter, fastq, readsPerBatch, chunk, blocks));
                return Figures{s.passedRecords, s.totalRecords, s.blockLines};
            }
            const BamSubsetStats s = native ? (device ? bamSubsetDevice(path, out, filter, readsPerBatch, chunk, walk, nullptr, BamOutputDeflate::Host, blocks)
                                                      : bamSubset(path, out, filter, readsPerBatch, chunk, blocks))
                                            : (device ? bamSubsetFastqDevice(path, out, filter, fastq, readsPerBatch, chunk, walk, nullptr, blocks)
                                                      : bamSubsetFastq(path, out, filter, fastq, readsPerBatch, chunk, blocks));
            return Figures{s.passedRecords, s.totalRecords, s.blockLines};
        };
        auto figures = [](const Figures &f) {
            char line[160];
            snprintf(line, sizeof line, "read subset: kept %llu of %llu records, %llu block lines.", (unsigned long long)f.kept, (unsigned long long)f.total,
                     (unsigned long long)f.blockLines);
            return std::string(line);
        };
        auto stats = [&]() {
            if (!wantStats) return;
            uint64_t sum[3] = {0, 0, 0};
            for (size_t w = 0; w < filter.deviceCount(); ++w) {
                uint64_t one[3] = {0, 0, 0};
                if (ts_read_fastq_text_stats(filter.context(w), one) == TS_OK) for (int j = 0; j < 3; ++j) sum[j] += one[j];
            }
            fprintf(stderr, "read fastq text: %llu calls, %llu records, %llu bytes\n", (unsigned long long)sum[0], (unsigned long long)sum[1], (unsigned long long)sum[2]);
        };
        if (!each.empty()) {
            std::ifstream list(each);
            std::string path;
            while (std::getline(list, path)) {
                if (path.empty()) continue;
                std::unique_ptr<std::ofstream> blocks;
                try {
                    std::ofstream out(path + ".out", std::ios::binary);
                    if (wantBlocks) blocks.reset(new std::ofstream(path + ".blocks", std::ios::binary));
                    const Figures f = subset(path, out, blocks.get());
                    out.close();
                    std::ofstream(path + ".ok") << figures(f) << "\n";
                } catch (const std::exception &e) {
                    std::rename((path + ".out").c_str(), (path + ".partial").c_str());     // (what was written before the failure)
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
            stats();
            return 0;
        }
        std::unique_ptr<std::ofstream> blocks;
        if (wantBlocks) {
            blocks.reset(new std::ofstream(blocksPath, std::ios::binary));
            if (!*blocks) throw std::runtime_error("cannot open '" + blocksPath + "'");
        }
        const Figures f = subset(input, std::cout, blocks.get());
        std::cout.flush();
        fprintf(stderr, "%s\n", figures(f).c_str());
        stats();
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
