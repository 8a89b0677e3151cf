// bam_deflate_cli.cpp — TEST INFRASTRUCTURE: --bam-subset through bamSubsetDevice of include/teloscope_mi355x_io.hpp with the
// output compressed by zlib on the host (--deflate host: the default, the bytes bam_device_cli --device writes) or by the
// device encoder (--deflate device: BamOutputDeflate::Device), on one context or several, so that the two can be compared on
// the same file by the same binary.
// Usage: bam_deflate_cli --bam-subset [--deflate host|device] [--devices 0,0] [--bam-chunk-bytes N] [--reads-per-batch N]
//                        [-c -p -x -l -y -k -d -t ...] file|-
//        bam_deflate_cli --bam-subset-each LIST ...  every file named in LIST through one filter: <file>.out and <file>.ok, or
//                                                    <file>.err with the message (the convention of bam_device_cli)
// stderr carries the reference's lines and one line of the library's counters (ts_bgzf_deflate_stats of every context, summed):
//   deflate: calls %llu members %llu plain %llu out %llu; route: plain %llu out %llu
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
    bool bamSubsetMode = false;
    BamOutputDeflate deflate = BamOutputDeflate::Host;
    size_t readsPerBatch = 1u << 20, bamChunk = size_t(256) << 20;
    std::vector<std::string> rawPatterns;
    std::vector<int> devices;
    bool hasPatterns = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) exit(EXIT_FAILURE); return argv[++i]; };
        if (a == "--bam-subset") bamSubsetMode = true;
        else if (a == "--bam-subset-each") { bamSubsetMode = true; bamList = val(); }
        else if (a == "--deflate") {
            const std::string v = val();
            if (v != "host" && v != "device") { fprintf(stderr, "bam_deflate_cli: --deflate host|device\n"); return EXIT_FAILURE; }
            deflate = v == "device" ? BamOutputDeflate::Device : BamOutputDeflate::Host;
        }
        else if (a == "--devices") { std::istringstream ds(val()); std::string d; while (std::getline(ds, d, ',')) if (!d.empty()) devices.push_back(std::stoi(d)); }
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
    if (!bamSubsetMode) { fprintf(stderr, "bam_deflate_cli: --bam-subset or --bam-subset-each is required\n"); return EXIT_FAILURE; }
    uint64_t routePlain = 0, routeOut = 0;
    auto subset = [&](const std::string &path, std::ostream &out, ReadTelomereFilter &filter) {
        const BamSubsetStats st = bamSubsetDevice(path, out, filter, readsPerBatch, bamChunk, BamRecordWalk::Index, nullptr, deflate);
        routePlain += st.deflatePlainBytes; routeOut += st.deflateMemberBytes;
        return st;
    };
    auto counters = [&](ReadTelomereFilter &filter) {
        uint64_t sum[4] = {0, 0, 0, 0};
        std::vector<ts_ctx *> seen;
        for (size_t w = 0; w < filter.deviceCount(); ++w) {
            ts_ctx *c = filter.context(w);
            bool dup = false;
            for (ts_ctx *s : seen) dup = dup || s == c;
            if (dup) continue;
            seen.push_back(c);
            uint64_t s[4];
            if (ts_bgzf_deflate_stats(c, s) == TS_OK) for (int i = 0; i < 4; ++i) sum[i] += s[i];
        }
        fprintf(stderr, "deflate: calls %llu members %llu plain %llu out %llu; route: plain %llu out %llu\n", (unsigned long long)sum[0],
                (unsigned long long)sum[1], (unsigned long long)sum[2], (unsigned long long)sum[3], (unsigned long long)routePlain,
                (unsigned long long)routeOut);
    };
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        std::unique_ptr<ReadTelomereFilter> made(devices.empty() ? new ReadTelomereFilter(ui) : new ReadTelomereFilter(ui, devices));
        ReadTelomereFilter &filter = *made;                     // (no device: throws — there is no host scan behind the route)
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
