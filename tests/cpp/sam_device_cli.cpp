// sam_device_cli.cpp — TEST INFRASTRUCTURE: --sam-subset of include/teloscope_mi355x_io.hpp on a ReadTelomereFilter of one or
// several contexts, through the host route (samSubset: lines and fields found on the host) or the device route (samSubsetDevice:
// lines and tabs indexed, lines cut and checked, sequences staged and passing lines gathered on the GPU), so that the two can be
// compared on the same input by the same binary.
// Usage: sam_device_cli --sam-subset [--device|--host] [--devices 0,0,0] [--chunk-bytes N] [--reads-per-batch N] [--figures]
//                       [-c -p -x -l -y -k -d -t ...] [file|-]          (no file: stdin)
//        --figures: the device route's per-context figures on stderr, a JSON line per context, before the closing line
//        sam_device_cli --sam-subset ... --each LIST   every file named in LIST through one filter: <file>.out and <file>.ok (the
//                                                      statistics), or <file>.err with the message and <file>.partial with what was
//                                                      written before it; a line "<file" puts the file on descriptor 0 and runs
//                                                      the route on "-"
//        sam_device_cli --dump-records FILE            no filter and no device: the host walk of the whole file (detail::samWalkHost)
//                                                      as text — the header extent, a line per record, the verdict
// stdout carries the subset.  stderr ends with "SAM subset: kept K of T records (M without sequence, H header lines)."; a failure
// is "Error: <message>" and exit status 1.
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

static int dumpRecords(const std::string &path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { fprintf(stderr, "Error: cannot open '%s'\n", path.c_str()); return EXIT_FAILURE; }
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    detail::SamWalk w;
    detail::samWalkHost(text.data(), text.size(), true, true, w);
    printf("header %llu %llu\n", (unsigned long long)w.headerLines, (unsigned long long)w.headerEnd);
    for (const ts_sam_record &r : w.recs)
        printf("record %llu %u %u %u %u\n", (unsigned long long)r.off, r.seq_at, r.seq_len, r.size, r.flags);
    printf("lines %llu next %llu error %d %llu %llu\n", (unsigned long long)w.lines, (unsigned long long)w.next, w.error,
           (unsigned long long)w.errorLine, (unsigned long long)w.errorOff);
    return 0;
}

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, each, dump;
    bool samSubsetMode = false, device = true, perContext = false;
    size_t readsPerBatch = 1u << 20, chunkBytes = 0;
    std::vector<int> devices;
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
        if (a == "--sam-subset") samSubsetMode = true;
        else if (a == "--dump-records") dump = val();
        else if (a == "--device") device = true;
        else if (a == "--host") device = false;
        else if (a == "--each") each = val();
        else if (a == "--figures") perContext = true;
        else if (a == "--devices") list(val(), [&](const std::string &x) { devices.push_back(std::stoi(x)); });
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
    if (!dump.empty()) return dumpRecords(dump);
    if (!samSubsetMode) { fprintf(stderr, "sam_device_cli: --sam-subset or --dump-records FILE is required\n"); return EXIT_FAILURE; }
    if (input.empty()) input = "-";
    try {
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui, devices);                 // (no device: throws — there is no host scan behind either route)
        filter.bindThreadToDevice();
        const size_t chunk = chunkBytes ? chunkBytes : size_t(256) << 20;
        std::vector<ReadRouteDeviceStats> per;
        auto subset = [&](const std::string &path, std::ostream &out) {
            return device ? samSubsetDevice(path, out, filter, readsPerBatch, chunk, perContext ? &per : nullptr) : samSubset(path, out, filter, readsPerBatch, chunk);
        };
        auto figures = [](const SamSubsetStats &s) {
            char line[200];
            snprintf(line, sizeof line, "SAM subset: kept %llu of %llu records (%llu without sequence, %llu header lines).", (unsigned long long)s.passedRecords,
                     (unsigned long long)s.totalRecords, (unsigned long long)s.missingSequenceRecords, (unsigned long long)s.headerLines);
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
                    std::ofstream out(path + ".out", std::ios::binary);
                    const SamSubsetStats s = subset(viaStdin ? "-" : path, out);
                    out.close();
                    std::ofstream(path + ".ok") << figures(s) << "\n";
                } catch (const std::exception &e) {
                    std::rename((path + ".out").c_str(), (path + ".partial").c_str());     // (what was written before the failure)
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
            return 0;
        }
        const SamSubsetStats s = subset(input, std::cout);
        std::cout.flush();
        for (const ReadRouteDeviceStats &c : per)
            fprintf(stderr, "{\"chunks\": %llu, \"recordsJudged\": %llu, \"bytesReceived\": %llu, \"msCommit\": %.3f, \"msCarryWait\": %.3f}\n",
                    (unsigned long long)c.chunks, (unsigned long long)c.recordsJudged, (unsigned long long)c.bytesReceived, c.msCommit, c.msCarryWait);
        fprintf(stderr, "%s\n", figures(s).c_str());
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
