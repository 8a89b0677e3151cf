// assembly_device_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of both routes of the assembly front ends with the reference's
// assembly record filters (include/teloscope_mi355x_filter.hpp), in one binary:
//   assembly_device_cli --device|--host <input> -o DIR [flags] [--include-bed F] [--exclude-bed F] [--include-prefix LIST]
//                       [--exclude-prefix LIST] [--chunk-bytes N] [--resident-limit N] [--times]
// --host is tests/cpp/assembly_cli.cpp's path (the default): the selection is resolved before any output file is made and before
// any device call, then scanFastaToFiles / annotateGfa.  --device hands the selector to scanFastaToFilesDevice /
// annotateGfaDevice, which resolve the selection over the text in device memory.  Both write the same files, the same stdout
// (FASTA: console report and summary; GFA: "segments ends scanned no_seq nodes parse_ms scan_ms write_ms") and the same
// "Sequence filter: ..." line on stderr, so that a test can hold every byte of one route against the other's.
//   --chunk-bytes n      the device route's chunk (the host route's FASTA group)
//   --resident-limit n   device route, FASTA: the most text that may be resident (a test hook)
//   --times              "library_bases N" on stderr: the bases handed to the library
//   --selection-only     host route: resolve and validate the selection, print "Sequence filter: ..." on stderr and every
//                        selected record on stdout (FASTA "index<TAB>id<TAB>bases<TAB>group", GFA "index<TAB>name"), then stop: no
//                        device is touched
// -j is accepted and ignored.  Errors go to stderr as "Error: <message>" with exit status 1.
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

}  // namespace

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".";
    std::vector<std::string> rawPatterns;
    bool hasPatterns = false, manualCuration = false, readSubset = false, selectionOnly = false, times = false;
    size_t chunkBytes = size_t(256) << 20;
    uint64_t residentLimit = 0;
    bool device = false;
    try {
        for (int i = 1; i < argc; ++i) {
            std::string a = argv[i], inlineValue;
            bool hasInline = false;
            if (a.compare(0, 2, "--") == 0 && a.find('=') != std::string::npos) {       // --option=value
                inlineValue = a.substr(a.find('=') + 1);
                a = a.substr(0, a.find('='));
                hasInline = true;
            }
            auto val = [&]() -> std::string {
                if (hasInline) return inlineValue;
                if (i + 1 >= argc) throw UsageError("Option " + a + " is missing a required argument");
                return argv[++i];
            };
            if (a == "--device") device = true;
            else if (a == "--host") device = false;
            else if (a == "--chunk-bytes") chunkBytes = static_cast<size_t>(std::stoull(val()));
            else if (a == "--resident-limit") residentLimit = std::stoull(val());
            else if (a == "-f") input = val();
            else if (a == "-o") outDir = val();
            else if (a == "-j") (void)val();
            else if (a == "--include-bed") addBedFilterFile(ui, val(), ui.includeBedFiles, "--include-bed");
            else if (a == "--exclude-bed") addBedFilterFile(ui, val(), ui.excludeBedFiles, "--exclude-bed");
            else if (a == "--include-prefix") addPrefixFilters(ui, val(), ui.includePrefixes, "--include-prefix");
            else if (a == "--exclude-prefix") addPrefixFilters(ui, val(), ui.excludePrefixes, "--exclude-prefix");
            else if (a == "--fastq-subset" || a == "--bam-subset") readSubset = true;
            else if (a == "--selection-only") selectionOnly = true;
            else if (a == "--times") times = true;
            else if (a == "-c") canonical = val();
            else if (a == "-p") {
                hasPatterns = true;
                std::istringstream ps(val());
                std::string p;
                while (std::getline(ps, p, ',')) if (!p.empty()) rawPatterns.push_back(p);
            }
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
        }
        if (ui.sequenceFilterActive && readSubset)
            throw UsageError("--include-bed/--exclude-bed/--include-prefix/--exclude-prefix filter assembly records and cannot be used in read subset mode.");
        if (readSubset) throw UsageError("read subset modes are driven by manifest_cli.");
        if (input.empty()) throw UsageError("No input file provided. Use -f or pass as positional argument.");
        if (ui.step > ui.windowSize) throw UsageError("Step size cannot be larger than window size.");

        const SequenceSelector selector(ui);                      // the selector files are read first, as Input::read does
        auto prepare = [&]() {                                    // (no device call before this)
            if (!canonical.empty()) setCanonical(ui, canonical);
            ui.rawPatterns = (hasPatterns && !rawPatterns.empty()) ? rawPatterns
                           : std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev};
            ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
            std::filesystem::create_directories(outDir);
        };
        const std::string name = std::filesystem::path(input).filename().string();

        if (device && selectionOnly) throw UsageError("--selection-only is the host route's.");
        if (isGfaAssemblyPath(input)) {
            GfaAnnotateStats st;
            if (device) {
                prepare();
                Teloscope teloscope(ui);
                st = annotateGfaDevice(teloscope, input, outDir, selector, std::cerr, chunkBytes);
            } else {
                if (selector.active()) validateFilteredGfa(input);
                const GfaGraph g = readGfa(input);
                const SequenceSelection sel = selectGfa(g, selector);
                if (selector.active()) std::cerr << selectionMessage(sel) << "\n";
                if (selectionOnly) {
                    for (size_t k = 0; k < sel.keep.size(); ++k)
                        if (sel.keep[k]) std::cout << k << "\t" << (g.paths.empty() ? g.segments[k].name : g.paths[k].name) << "\n";
                    return 0;
                }
                prepare();
                Teloscope teloscope(ui);
                st = annotateGfa(teloscope, g, &sel, outDir);
            }
            std::cout << st.segments << " " << st.ends << " " << st.scanned << " " << st.noSeq << " " << st.nodes << " "
                      << st.parseMs << " " << st.scanMs << " " << st.writeMs << "\n";
            return 0;
        }

        const std::string outBase = outDir + "/" + name;
        ScanFastaTimes T;
        if (device) {
            prepare();
            Teloscope teloscope(ui);
            teloscope.bindThreadToDevice();
            const AssemblySummary summary = scanFastaToFilesDevice(teloscope, input, outBase, std::cout, manualCuration, chunkBytes, &T,
                                                                   0xfffffffeull, false, &selector, std::cerr, residentLimit);
            printSummary(std::cout, summary, ui.ultraFastMode, outBase + "_report.tsv");
            if (times) std::fprintf(stderr, "library_bases %llu\n", static_cast<unsigned long long>(T.library_bases));
            return 0;
        }
        FastaGroupReader reader(input, chunkBytes, size_t(4) << 20, true, selector.active());
        if (selector.active()) {
            const SequenceSelection sel = selector.select(reader.primaryIds(), "paths");
            reader.keep(sel.keep);
            ui.filterInputCount = sel.inputCount;
            ui.filterSelectedCount = sel.selectedCount;
            std::cerr << selectionMessage(sel) << "\n";
        }
        if (selectionOnly) {
            detail::FastaGroup grp;
            for (size_t k = 0; reader.next(grp); ++k) {
                for (size_t r = 0; r < grp.records.size(); ++r)
                    std::cout << grp.seqPos[r] << "\t" << grp.records[r].header << "\t" << grp.records[r].size << "\t" << k << "\n";
                for (size_t r = 0; r < grp.owned.size(); ++r)
                    std::cout << grp.seqPos[r] << "\t" << grp.owned[r].header << "\t" << grp.owned[r].sequence.size() << "\t" << k << "\n";
            }
            return 0;
        }
        prepare();
        Teloscope teloscope(ui);
        teloscope.bindThreadToDevice();
        const AssemblySummary summary = scanFastaToFiles(teloscope, input, outBase, std::cout, manualCuration, chunkBytes, &T,
                                                         size_t(4) << 20, -1, &reader);
        printSummary(std::cout, summary, ui.ultraFastMode, outBase + "_report.tsv");
        if (times) std::fprintf(stderr, "library_bases %llu\n", static_cast<unsigned long long>(T.library_bases));
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
    return 0;
}
