// bam_index_cli.cpp — TEST INFRASTRUCTURE: --bam-subset through the device route of include/teloscope_mi355x_io.hpp
// (bamSubsetDevice) with either record walk, the serial one (ts_bam_chunk_walk) or the parallel index (ts_bam_chunk_index), or
// through the host route (bamSubset), so that the three can be compared on the same file by the same binary.
// Usage: bam_index_cli --bam-subset [--walk serial|index] [--host] [--bam-chunk-bytes N] [--reads-per-batch N]
//                      [-c -p -x -l -y -k -d -t ...] file|-
//        bam_index_cli --bam-subset-each LIST ...    every file named in LIST through one filter: <file>.out and <file>.ok, or
//                                                    <file>.err with the message (the convention of manifest_cli)
// stderr carries the reference's lines ("BAM subset: kept %d of %d records.", "... skipped %d record(s) without SEQ.") and, last,
// the library's counters (ts_bam_index_stats):
//   "bam index: calls C entered E hits H settled S records R row bytes B"
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
    std::string input, canonical, bamList;
    bool bamSubsetMode = false, device = true;
    BamRecordWalk walk = BamRecordWalk::Serial;
    size_t readsPerBatch = 1u << 20, bamChunk = size_t(256) << 20;
    std::vector<std::string> rawPatterns;
    bool hasPatterns = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) exit(EXIT_FAILURE); return argv[++i]; };
        if (a == "--bam-subset") bamSubsetMode = true;
        else if (a == "--bam-subset-each") { bamSubsetMode = true; bamList = val(); }
        else if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--walk") {
            const std::string w = val();
            if (w != "serial" && w != "index") { fprintf(stderr, "bam_index_cli: --walk serial|index\n"); return EXIT_FAILURE; }
            walk = w == "index" ? BamRecordWalk::Index : BamRecordWalk::Serial;
        }
        else if (a == "--reads-per-batch") readsPerBatch = static_cast<size_t>(std::stoull(val()));
        else if (a == "--bam-chunk-bytes") bamChunk = static_cast<size_t>(std::stoull(val()));
        else if (a == "-f") input = val();
        else if (a == "-c") canonical = val();
        else if (a == "-p") {
            hasPatterns = true;
            std::istringstream ps(val());
            std::string p;
            while (std::getline(ps, p, ',')) if (!p.empty()) rawPatterns.push_back(p);
        }
        else if (a == "-t") ui.terminalLimit = std::stoi(val());
        else if (a == "-k") ui.maxMatchDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-d") ui.maxBlockDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-l") { ui.minBlockLen = static_cast<unsigned short>(std::stoi(val())); ui.minBlockLenSet = true; }
        else if (a == "-y") ui.minBlockDensity = std::stof(val());
        else if (a == "-x") ui.editDistance = static_cast<uint8_t>(std::stoi(val()));
        else if (!a.empty() && (a[0] != '-' || a == "-") && input.empty()) input = a;
    }
    if (!bamSubsetMode) { fprintf(stderr, "bam_index_cli: --bam-subset or --bam-subset-each is required\n"); return EXIT_FAILURE; }
    auto subset = [&](const std::string &path, std::ostream &out, ReadTelomereFilter &filter) {
        return device ? bamSubsetDevice(path, out, filter, readsPerBatch, bamChunk, walk) : bamSubset(path, out, filter, readsPerBatch, bamChunk);
    };
    auto counters = [](ReadTelomereFilter &filter) {
        uint64_t s[6] = {0, 0, 0, 0, 0, 0};
        ts_bam_index_stats(filter.context(0), s);
        fprintf(stderr, "bam index: calls %llu entered %llu hits %llu settled %llu records %llu row bytes %llu\n", (unsigned long long)s[0],
                (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3], (unsigned long long)s[4], (unsigned long long)s[5]);
    };
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui);                          // (no device: throws — there is no host scan behind either route)
        filter.bindThreadToDevice();
        if (!bamList.empty()) {
            std::ifstream list(bamList);
            std::string path;
            while (std::getline(list, path)) {
                if (path.empty()) continue;
                try {
                    std::ofstream out(path + ".out", std::ios::binary);
                    const BamSubsetStats st = subset(path, out, filter);
                    out.close();
                    std::ofstream(path + ".ok") << st.passedRecords << " " << st.totalRecords << " " << (st.missingEofBlock ? 1 : 0) << "\n";
                } catch (const std::exception &e) {
                    std::remove((path + ".out").c_str());
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
            counters(filter);
            return 0;
        }
        const BamSubsetStats st = subset(input.empty() ? "-" : input, std::cout, filter);
        if (st.missingEofBlock) fprintf(stderr, "Warning: BAM input is missing the BGZF EOF marker.\n");
        if (st.missingSequenceRecords)
            fprintf(stderr, "BAM subset: skipped %llu record%s without SEQ.\n", (unsigned long long)st.missingSequenceRecords,
                    st.missingSequenceRecords == 1 ? "" : "s");
        fprintf(stderr, "BAM subset: kept %llu of %llu records.\n", (unsigned long long)st.passedRecords, (unsigned long long)st.totalRecords);
        counters(filter);
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
