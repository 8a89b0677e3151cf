// assembly_routes_multi_cli.cpp — TEST INFRASTRUCTURE: the two assembly front ends of include/teloscope_mi355x_io.hpp and
// include/teloscope_mi355x_gfa.hpp on a Teloscope of one or several contexts, through the host route (scanFastaToFiles /
// annotateGfa: a batch's segments sharded over the contexts) or the device route (scanFastaToFilesDevice / annotateGfaDevice: the
// input's chunks dealt to the contexts), so that every combination can be compared on the same input by the same binary.
// Usage: assembly_routes_multi_cli --fasta|--gfa --device|--host [--devices 0,0,0] [--chunk-bytes N] [--device-tracks]
//                                  [--chunk-limit N] [--include-bed F] [--exclude-bed F] [--include-prefix LIST]
//                                  [--exclude-prefix LIST] [-c -p -w -s -t -k -d -l -y -x -r -g -e -m -i -a -u -n] -o DIR INPUT
//        assembly_routes_multi_cli ... -o DIR --each LIST   every file named in LIST (one path per line) through ONE Teloscope in
//                                  one process; a file that fails prints its error and the run goes on (exit status 1)
//   --devices       the HIP ordinals the Teloscope is made over (an ordinal may repeat: several contexts share that GPU); it is
//                   made with DeviceRoutes::EveryContext, so the device routes use all of them
//   --chunk-bytes   the device route's chunk (the host FASTA route's group); a list N,N,... runs every file at each size in
//                   turn, the sizes outermost, size N's outputs under DIR/cN/
//   --device-tracks FASTA, device route: the window tracks and, under -m, the match files are formatted on the device
//   --chunk-limit   FASTA, device route: the most a device chunk may grow to (a test hook)
// FASTA writes DIR/<name>_*.bed / .bedgraph / _report.tsv (with --each: DIR/<k>.<name>_*) and the console report + summary on
// stdout; GFA writes DIR/<name>.telo.annotated.gfa and .colors.csv (with --each: under DIR/<k>/) and "segments ends scanned no_seq
// nodes" on stdout.  stderr carries one JSON line per file: the summary or stats struct, the deterministic fields of
// ScanFastaTimes, the text the route wrote to its log (warnings, the "Sequence filter:" line), and for the device routes
// `contexts`: one object per context (AssemblyRouteDeviceStats, and what terminalEndsStats of that context moved by).  On an
// exception it prints "Error: <message>" (with --each "Error: <file name>: <message>", and a JSON line with "error") and exits 1.
// -j is accepted and ignored.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_filter.hpp"
#include "teloscope_mi355x_gfa.hpp"
#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

namespace {

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

const char *kHelp =
    "assembly_routes_multi_cli --fasta|--gfa --device|--host [--devices 0,0,0] [--chunk-bytes N] [--device-tracks] [--chunk-limit N]\n"
    "                          [--include-bed F] [--exclude-bed F] [--include-prefix LIST] [--exclude-prefix LIST]\n"
    "                          [-c -p -w -s -t -k -d -l -y -x -r -g -e -m -i -a -u -n] -o DIR (INPUT | --each LIST)\n";

std::string jsonString(const std::string &s) {
    std::string out = "\"";
    for (unsigned char c : s) {
        char b[8];
        if (c == '"' || c == '\\') { out += '\\'; out += static_cast<char>(c); }
        else if (c < 0x20 || c >= 0x7f) { std::snprintf(b, sizeof b, "\\u%04x", c); out += b; }
        else out += static_cast<char>(c);
    }
    return out + "\"";
}

std::string contextsJson(const std::vector<AssemblyRouteDeviceStats> &per, const std::vector<std::array<uint64_t, 4>> &endsMoved) {
    std::string out;
    for (size_t w = 0; w < per.size(); ++w) {
        const AssemblyRouteDeviceStats &s = per[w];
        const std::array<uint64_t, 4> e = w < endsMoved.size() ? endsMoved[w] : std::array<uint64_t, 4>{};
        char line[768];
        std::snprintf(line, sizeof line, "%s{\"device\": %d, \"chunks\": %llu, \"records\": %llu, \"basesScanned\": %llu, \"bytesReceived\": %llu, "
                      "\"msFill\": %.3f, \"msStage\": %.3f, \"msFrameWait\": %.3f, \"msCommit\": %.3f, \"msIndex\": %.3f, \"msJoin\": %.3f, \"msScan\": %.3f, "
                      "\"terminalEnds\": [%llu, %llu, %llu, %llu]}", out.empty() ? "" : ", ", s.device, (unsigned long long)s.chunks,
                      (unsigned long long)s.records, (unsigned long long)s.basesScanned, (unsigned long long)s.bytesReceived, s.msFill, s.msStage,
                      s.msFrameWait, s.msCommit, s.msIndex, s.msJoin, s.msScan, (unsigned long long)e[0], (unsigned long long)e[1],
                      (unsigned long long)e[2], (unsigned long long)e[3]);
        out += line;
    }
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".", eachList;
    std::vector<std::string> rawPatterns;
    std::vector<int> devices;
    bool hasPatterns = false, manualCuration = false, deviceTracks = false;
    int format = -1, route = -1;                                 // 1 FASTA, 0 GFA; 1 device, 0 host
    std::vector<size_t> chunkSizes;
    uint64_t chunkLimit = 0xfffffffeull;
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string {
                if (i + 1 >= argc) throw UsageError("Option " + a + " is missing a required argument");
                return argv[++i];
            };
            auto list = [&](const std::string &v, auto &&one) {
                std::istringstream in(v);
                std::string x;
                while (std::getline(in, x, ',')) if (!x.empty()) one(x);
            };
            if (a == "--help" || a == "-h") { std::fputs(kHelp, stdout); return 0; }
            else if (a == "--fasta") format = 1;
            else if (a == "--gfa") format = 0;
            else if (a == "--device") route = 1;
            else if (a == "--host") route = 0;
            else if (a == "--devices") list(val(), [&](const std::string &x) { devices.push_back(std::stoi(x)); });
            else if (a == "--chunk-bytes") list(val(), [&](const std::string &x) { chunkSizes.push_back(static_cast<size_t>(std::stoull(x))); });
            else if (a == "--chunk-limit") chunkLimit = std::stoull(val());
            else if (a == "--device-tracks") deviceTracks = true;
            else if (a == "--each") eachList = val();
            else if (a == "--include-bed") addBedFilterFile(ui, val(), ui.includeBedFiles, "--include-bed");
            else if (a == "--exclude-bed") addBedFilterFile(ui, val(), ui.excludeBedFiles, "--exclude-bed");
            else if (a == "--include-prefix") addPrefixFilters(ui, val(), ui.includePrefixes, "--include-prefix");
            else if (a == "--exclude-prefix") addPrefixFilters(ui, val(), ui.excludePrefixes, "--exclude-prefix");
            else if (a == "-f") input = val();
            else if (a == "-o") outDir = val();
            else if (a == "-j") (void)val();
            else if (a == "-c") canonical = val();
            else if (a == "-p") { hasPatterns = true; list(val(), [&](const std::string &x) { rawPatterns.push_back(x); }); }
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
        if (format < 0) throw UsageError("one of --fasta and --gfa is required");
        if (route < 0) throw UsageError("one of --device and --host is required");
        std::vector<std::string> inputs;
        if (!eachList.empty()) {
            std::ifstream in(eachList);
            if (!in) throw UsageError("cannot open the list " + eachList);
            for (std::string line; std::getline(in, line);) if (!line.empty()) inputs.push_back(line);
        } else if (!input.empty()) inputs.push_back(input);
        if (inputs.empty()) throw UsageError("No input file provided.");
        if (ui.step > ui.windowSize) throw UsageError("Step size cannot be larger than window size.");

        const SequenceSelector selector(ui);                      // the selector files are read first, as Input::read does
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        Teloscope teloscope(ui, devices, DeviceRoutes::EveryContext);
        const char *routeName = route == 1 ? "device" : "host";
        int status = 0;
        const bool manySizes = chunkSizes.size() > 1;
        if (chunkSizes.empty()) chunkSizes.push_back(size_t(256) << 20);
        const std::string outRoot = outDir;
        for (const size_t chunkBytes : chunkSizes)
        for (size_t k = 0; k < inputs.size(); ++k) {
            const std::string outDir = manySizes ? outRoot + "/c" + std::to_string(chunkBytes) : outRoot;
            const std::string name = std::filesystem::path(inputs[k]).filename().string();
            std::ostringstream log;
            std::vector<AssemblyRouteDeviceStats> per;
            std::vector<std::array<uint64_t, 4>> endsBefore, endsMoved;
            for (size_t w = 0; w < teloscope.deviceCount(); ++w) endsBefore.push_back(teloscope.terminalEndsStats(w));
            auto moved = [&]() {
                for (size_t w = 0; w < teloscope.deviceCount(); ++w) {
                    std::array<uint64_t, 4> now = teloscope.terminalEndsStats(w);
                    for (size_t j = 0; j < 4; ++j) now[j] -= endsBefore[w][j];
                    endsMoved.push_back(now);
                }
            };
            try {
                std::string result;
                if (format == 0) {
                    const std::string dir = eachList.empty() ? outDir : outDir + "/" + std::to_string(k);
                    std::filesystem::create_directories(dir);
                    const GfaAnnotateStats st = route == 1 ? annotateGfaDevice(teloscope, inputs[k], dir, selector, log, chunkBytes, &per)
                                                           : annotateGfa(teloscope, inputs[k], dir, selector, log);
                    std::cout << st.segments << " " << st.ends << " " << st.scanned << " " << st.noSeq << " " << st.nodes << std::endl;
                    result = "\"stats\": {\"segments\": " + std::to_string(st.segments) + ", \"ends\": " + std::to_string(st.ends) + ", \"scanned\": " +
                             std::to_string(st.scanned) + ", \"noSeq\": " + std::to_string(st.noSeq) + ", \"nodes\": " + std::to_string(st.nodes) + "}";
                } else {
                    std::filesystem::create_directories(outDir);
                    const std::string outBase = outDir + "/" + (eachList.empty() ? name : std::to_string(k) + "." + name);
                    ScanFastaTimes T;
                    AssemblySummary summary;
                    if (route == 1) {
                        summary = scanFastaToFilesDevice(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes, &T, chunkLimit, deviceTracks,
                                                         &selector, log, 0, &per);
                    } else {
                        // (the filtered host route resolves its selection before the Teloscope exists: tests/cpp/assembly_device_cli.cpp drives it)
                        if (selector.active()) throw UsageError("FASTA with assembly record filters on the host route is assembly_device_cli's");
                        summary = scanFastaToFiles(teloscope, inputs[k], outBase, std::cout, manualCuration, chunkBytes, &T);
                    }
                    printSummary(std::cout, summary, ui.ultraFastMode, outBase + "_report.tsv");
                    std::cout.flush();
                    result = "\"summary\": {\"totalPaths\": " + std::to_string(summary.totalPaths) + ", \"totalTelomeres\": " + std::to_string(summary.totalTelomeres) +
                             ", \"totalGaps\": " + std::to_string(summary.totalGaps) + ", \"totalITS\": " + std::to_string(summary.totalITS) +
                             ", \"totalCanMatches\": " + std::to_string(summary.totalCanMatches) + ", \"totalNWindows\": " + std::to_string(summary.totalNWindows) +
                             ", \"filterActive\": " + (summary.filterActive ? "true" : "false") + ", \"filterInputCount\": " + std::to_string(summary.filterInputCount) +
                             ", \"filterSelectedCount\": " + std::to_string(summary.filterSelectedCount) + "}, \"times\": {\"bases\": " + std::to_string(T.bases) +
                             ", \"windows\": " + std::to_string(T.windows) + ", \"library_bases\": " + std::to_string(T.library_bases) + ", \"groups\": " +
                             std::to_string(T.groups) + ", \"bases_read_back\": " + std::to_string(T.bases_read_back) + "}";
                }
                moved();
                std::fprintf(stderr, "{\"file\": %s, \"format\": \"%s\", \"route\": \"%s\", \"chunkBytes\": %zu, %s, \"log\": %s, \"contexts\": [%s]}\n", jsonString(name).c_str(),
                             format ? "fasta" : "gfa", routeName, chunkBytes, result.c_str(), jsonString(log.str()).c_str(), contextsJson(per, endsMoved).c_str());
            } catch (const std::exception &e) {
                std::fflush(stdout);
                std::cout.flush();
                if (eachList.empty()) throw;
                std::fprintf(stderr, "Error: %s: %s\n", name.c_str(), e.what());
                std::fprintf(stderr, "{\"file\": %s, \"format\": \"%s\", \"route\": \"%s\", \"chunkBytes\": %zu, \"error\": %s, \"log\": %s}\n", jsonString(name).c_str(),
                             format ? "fasta" : "gfa", routeName, chunkBytes, jsonString(e.what()).c_str(), jsonString(log.str()).c_str());
                status = EXIT_FAILURE;
            }
        }
        return status;
    } catch (const UsageError &e) {
        std::fprintf(stderr, "Error: %s\n%s", e.what(), kHelp);
        return EXIT_FAILURE;
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
