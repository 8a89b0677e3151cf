// read_routes_multi_cli.cpp — TEST INFRASTRUCTURE: --fastq-subset and --bam-subset of include/teloscope_mi355x_io.hpp on a
// ReadTelomereFilter of one or several contexts, through the host route (fastqSubset / bamSubset: a batch's reads sharded over the
// contexts) or the device route (fastqSubsetDevice / bamSubsetDevice: the input's chunks dealt to the contexts), so that every
// combination can be compared on the same input by the same binary.
// Usage: read_routes_multi_cli --fastq-subset|--bam-subset [--device|--host] [--devices 0,0,0] [--chunk-bytes N]
//                              [--reads-per-batch N] [--walk serial|index] [-c -p -x -l -y -k -d -t ...] [file|-]   (no file: stdin)
//        read_routes_multi_cli ... --each LIST   every file named in LIST through one filter: <file>.out and <file>.ok (the
//                                                result struct), or <file>.err with the message and <file>.partial with what was written before it;
//                                                a line "<file" puts the file on descriptor 0 and runs the route on "-"
// stdout carries the subset.  stderr ends with one JSON line: the result struct and, for the device routes, one object per context
// (ReadRouteDeviceStats); a failure is "Error: <message>" and exit status 1.
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
    std::string input, canonical, each;
    bool fastq = false, bam = false, device = true;
    size_t readsPerBatch = 1u << 20, chunkBytes = 0;
    BamRecordWalk walk = BamRecordWalk::Index;
    std::vector<int> devices;
    std::vector<std::string> rawPatterns;
    bool hasPatterns = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) exit(EXIT_FAILURE); return argv[++i]; };
        auto list = [&](const std::string &v, auto &&each) {
            std::istringstream in(v);
            std::string x;
            while (std::getline(in, x, ',')) if (!x.empty()) each(x);
        };
        if (a == "--fastq-subset") fastq = true;
        else if (a == "--bam-subset") bam = true;
        else if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--each") each = val();
        else if (a == "--devices") list(val(), [&](const std::string &x) { devices.push_back(std::stoi(x)); });
        else if (a == "--reads-per-batch") readsPerBatch = static_cast<size_t>(std::stoull(val()));
        else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
        else if (a == "--walk") {
            const std::string w = val();
            if (w != "serial" && w != "index") { fprintf(stderr, "read_routes_multi_cli: --walk serial|index\n"); return EXIT_FAILURE; }
            walk = w == "serial" ? BamRecordWalk::Serial : BamRecordWalk::Index;
        }
        else if (a == "-c") canonical = val();
        else if (a == "-p") { hasPatterns = true; list(val(), [&](const std::string &x) { rawPatterns.push_back(x); }); }
        else if (a == "-t") ui.terminalLimit = std::stoi(val());
        else if (a == "-k") ui.maxMatchDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-d") ui.maxBlockDist = static_cast<unsigned short>(std::stoi(val()));
        else if (a == "-l") { ui.minBlockLen = static_cast<unsigned short>(std::stoi(val())); ui.minBlockLenSet = true; }
        else if (a == "-y") ui.minBlockDensity = std::stof(val());
        else if (a == "-x") ui.editDistance = static_cast<uint8_t>(std::stoi(val()));
        else if (!a.empty() && (a[0] != '-' || a == "-") && input.empty()) input = a;
    }
    if (fastq == bam) { fprintf(stderr, "read_routes_multi_cli: one of --fastq-subset and --bam-subset is required\n"); return EXIT_FAILURE; }
    if (input.empty()) input = "-";
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui, devices);                 // (no device: throws — there is no host scan behind any route)
        filter.bindThreadToDevice();
        std::vector<ReadRouteDeviceStats> per;
        const size_t chunk = chunkBytes ? chunkBytes : size_t(256) << 20;
        auto subset = [&](const std::string &path, std::ostream &out) -> std::string {       // -> the result struct's fields
            if (fastq) {
                const FastqSubsetResult r = device ? fastqSubsetDevice(path, out, filter, readsPerBatch, chunk, &per)
                                                   : fastqSubset(path, out, filter, readsPerBatch, chunk);
                return "\"kept\": " + std::to_string(r.kept) + ", \"total\": " + std::to_string(r.total);
            }
            const BamSubsetStats s = device ? bamSubsetDevice(path, out, filter, readsPerBatch, chunk, walk, &per)
                                            : bamSubset(path, out, filter, readsPerBatch, chunk);
            return "\"totalRecords\": " + std::to_string(s.totalRecords) + ", \"passedRecords\": " + std::to_string(s.passedRecords) +
                   ", \"missingSequenceRecords\": " + std::to_string(s.missingSequenceRecords) + ", \"missingEofBlock\": " + (s.missingEofBlock ? "true" : "false");
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
                    std::ofstream out(path + ".out", std::ios::binary);
                    const std::string r = subset(viaStdin ? "-" : path, out);
                    out.close();
                    std::ofstream(path + ".ok") << r << "\n";
                } catch (const std::exception &e) {
                    std::rename((path + ".out").c_str(), (path + ".partial").c_str());     // (what was written before the failure)
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
            return 0;
        }
        const std::string result = subset(input, std::cout);
        std::cout.flush();
        std::string contexts;
        for (const ReadRouteDeviceStats &s : per) {
            char line[512];
            snprintf(line, sizeof line, "%s{\"chunks\": %llu, \"recordsJudged\": %llu, \"bytesReceived\": %llu, \"msSource\": %.3f, \"msCarryWait\": %.3f, "
                     "\"msCommit\": %.3f, \"msWalk\": %.3f, \"msStage\": %.3f, \"msFilter\": %.3f, \"msGather\": %.3f}", contexts.empty() ? "" : ", ",
                     (unsigned long long)s.chunks, (unsigned long long)s.recordsJudged, (unsigned long long)s.bytesReceived, s.msSource, s.msCarryWait,
                     s.msCommit, s.msWalk, s.msStage, s.msFilter, s.msGather);
            contexts += line;
        }
        fprintf(stderr, "{\"route\": \"%s\", \"device\": %s, \"result\": {%s}, \"contexts\": [%s]}\n", fastq ? "fastq-subset" : "bam-subset",
                device ? "true" : "false", result.c_str(), contexts.c_str());
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
