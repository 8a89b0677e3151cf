// gfa_device_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of the two routes of the GFA annotation,
//   gfa_device_cli --device|--host [--chunk-bytes N] [--devices LIST] [gfa_cli's flags] -o DIR -f INPUT
//   gfa_device_cli --device|--host ... -o DIR --each LIST
//   gfa_device_cli --dump-records INPUT
// --host is annotateGfa, --device annotateGfaDevice (include/teloscope_mi355x_gfa.hpp); both write DIR/<name>.telo.annotated.gfa
// and .colors.csv and print "segments ends scanned no_seq nodes parse_ms scan_ms write_ms" on stdout, warnings on stderr, so that
// a test can hold every byte of one route against the other's.  --each LIST: LIST is a text file with one input path per line;
// every file goes through ONE Teloscope in one process, file k's outputs under DIR/<k>; a file that fails prints its error and
// the run goes on (exit status 1).  --chunk-bytes is the device route's chunk, --devices the HIP ordinals the Teloscope is made
// over (an ordinal may repeat).
// --dump-records INPUT touches no device: readGfa's view of the file —
//   version <TAB> v <TAB> hasVersion
//   S <TAB> name <TAB> sequence length or * <TAB> FNV-1a 64 of the sequence (hex)
//   P <TAB> name { <TAB> component <TAB> orientation }
//   E <TAB> offset <TAB> length <TAB> replacement text
// or, when readGfa throws, error <TAB> its message.
// -j is accepted and ignored.  Errors go to stderr as "Error: <message>" with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_gfa.hpp"

using namespace teloscope_mi355x;

namespace {

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

int dumpRecords(const std::string &file) {
    try {
        const GfaGraph g = readGfa(file);
        std::cout << "version\t" << g.version << "\t" << (g.hasVersion ? 1 : 0) << "\n";
        for (const GfaSegment &s : g.segments) {
            uint64_t h = 0xcbf29ce484222325ull;
            for (uint64_t i = 0; s.seq && i < s.len; ++i) { h ^= static_cast<unsigned char>(s.seq[i]); h *= 0x100000001b3ull; }
            char hex[17];
            std::snprintf(hex, sizeof hex, "%016llx", static_cast<unsigned long long>(h));
            std::cout << "S\t" << s.name << "\t";
            if (s.seq) std::cout << s.len; else std::cout << "*";
            std::cout << "\t" << hex << "\n";
        }
        for (const GfaPath &p : g.paths) {
            std::cout << "P\t" << p.name;
            for (const auto &c : p.comps) std::cout << "\t" << c.first << "\t" << c.second;
            std::cout << "\n";
        }
        for (const GfaEdit &e : g.edits) std::cout << "E\t" << e.off << "\t" << e.len << "\t" << e.text << "\n";
    } catch (const std::exception &e) {
        std::cout << "error\t" << e.what() << "\n";
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".", eachList, dumpFile;
    std::vector<std::string> rawPatterns;
    std::vector<int> devices;
    int route = -1;                                              // 1 device, 0 host
    size_t chunkBytes = size_t(256) << 20;
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
            else if (!a.empty() && a[0] != '-' && input.empty()) input = a;
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
        if (!canonical.empty()) setCanonical(ui, canonical);
        ui.rawPatterns = rawPatterns.empty() ? std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev} : rawPatterns;
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        Teloscope teloscope(ui, devices);
        int status = 0;
        for (size_t k = 0; k < inputs.size(); ++k) {
            const std::string dir = eachList.empty() ? outDir : outDir + "/" + std::to_string(k);
            try {
                std::filesystem::create_directories(dir);
                const GfaAnnotateStats st = route == 1 ? annotateGfaDevice(teloscope, inputs[k], dir, std::cerr, chunkBytes)
                                                       : annotateGfa(teloscope, inputs[k], dir);
                std::cout << st.segments << " " << st.ends << " " << st.scanned << " " << st.noSeq << " " << st.nodes << " "
                          << st.parseMs << " " << st.scanMs << " " << st.writeMs << std::endl;
            } catch (const std::exception &e) {
                if (eachList.empty()) throw;
                std::cerr << "Error: " << std::filesystem::path(inputs[k]).filename().string() << ": " << e.what() << std::endl;
                status = EXIT_FAILURE;
            }
        }
        return status;
    } catch (const std::exception &e) {
        std::cout.flush();
        std::cerr << "Error: " << e.what() << "\n";
        return EXIT_FAILURE;
    }
}
