// read_blocks_cli.cpp — TEST INFRASTRUCTURE: the three read subsets of include/teloscope_mi355x_io.hpp with their read block
// report (the trailing `blocks` stream of fastqSubset / bamSubset / samSubset and of their device forms), on a ReadTelomereFilter of
// one or several contexts, so that host and device routes can be compared on the same input by the same binary.
// Usage: read_blocks_cli --fastq-subset|--bam-subset|--sam-subset [--host|--device] [--blocks FILE] [--contexts N]
//                        [--chunk-bytes N] [--reads-per-batch N] [--bam-walk serial|index] [--bam-deflate host|device] [--stats]
//                        [-c -p -x -l -y -k -d -t ...] [file|-]          (no file: stdin)
//        read_blocks_cli ... --each LIST   every file named in LIST through one filter: <file>.out and <file>.ok (the statistics),
//                                          or <file>.err with the message and <file>.partial with what was written before it; with
//                                          --blocks (its FILE is not used then) the report goes to <file>.blocks, also before a
//                                          failure; a line "<file" puts the file on descriptor 0 and runs the route on "-"
// stdout carries the subset.  stderr ends with "read subset: kept K of T records, B block lines."; --stats adds
// "read block text: C calls, L lines, B bytes" (ts_read_block_text_stats, summed over the contexts).  A failure is
// "Error: <message>" and exit status 1.
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
    bool device = true, wantBlocks = false, wantStats = false;
    size_t readsPerBatch = 1u << 20, chunkBytes = 0, contexts = 1;
    BamRecordWalk walk = BamRecordWalk::Index;
    BamOutputDeflate deflate = BamOutputDeflate::Host;
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
        if (a == "--fastq-subset" || a == "--bam-subset" || a == "--sam-subset") mode = a;
        else if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--blocks") { blocksPath = val(); wantBlocks = true; }
        else if (a == "--stats") wantStats = true;
        else if (a == "--each") each = val();
        else if (a == "--contexts") contexts = static_cast<size_t>(std::stoull(val()));
        else if (a == "--reads-per-batch") readsPerBatch = static_cast<size_t>(std::stoull(val()));
        else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
        else if (a == "--bam-walk") walk = val() == "serial" ? BamRecordWalk::Serial : BamRecordWalk::Index;
        else if (a == "--bam-deflate") deflate = val() == "device" ? BamOutputDeflate::Device : BamOutputDeflate::Host;
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
    if (mode.empty()) { fprintf(stderr, "read_blocks_cli: --fastq-subset, --bam-subset or --sam-subset is required\n"); return EXIT_FAILURE; }
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
            if (mode == "--fastq-subset") {
                const FastqSubsetResult r = device ? fastqSubsetDevice(path, out, filter, readsPerBatch, chunk, nullptr, blocks)
                                                   : fastqSubset(path, out, filter, readsPerBatch, chunk, blocks);
                return Figures{r.kept, r.total, r.blockLines};
            }
            if (mode == "--sam-subset") {
                const SamSubsetStats s = device ? samSubsetDevice(path, out, filter, readsPerBatch, chunk, nullptr, blocks)
                                                : samSubset(path, out, filter, readsPerBatch, chunk, blocks);
                return Figures{s.passedRecords, s.totalRecords, s.blockLines};
            }
            const BamSubsetStats s = device ? bamSubsetDevice(path, out, filter, readsPerBatch, chunk, walk, nullptr, deflate, blocks)
                                            : bamSubset(path, out, filter, readsPerBatch, chunk, blocks);
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
                if (ts_read_block_text_stats(filter.context(w), one) == TS_OK) for (int j = 0; j < 3; ++j) sum[j] += one[j];
            }
            fprintf(stderr, "read block text: %llu calls, %llu lines, %llu bytes\n", (unsigned long long)sum[0], (unsigned long long)sum[1], (unsigned long long)sum[2]);
        };
        if (!each.empty()) {
            std::ifstream list(each);
            std::string path;
            while (std::getline(list, path)) {
                if (path.empty()) continue;
                const bool viaStdin = path[0] == '<';
                if (viaStdin) path.erase(0, 1);
                std::unique_ptr<std::ofstream> blocks;
                try {
                    if (viaStdin) {
                        const int fd = ::open(path.c_str(), O_RDONLY);
                        if (fd < 0 || ::dup2(fd, 0) < 0) throw std::runtime_error("cannot put '" + path + "' on stdin");
                        if (fd != 0) ::close(fd);
                    }
                    std::ofstream out(path + ".out", std::ios::binary);
                    if (wantBlocks) blocks.reset(new std::ofstream(path + ".blocks", std::ios::binary));
                    const Figures f = subset(viaStdin ? "-" : path, out, blocks.get());
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
