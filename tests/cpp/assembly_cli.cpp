// assembly_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of the assembly front ends with the reference's assembly record filters
// (include/teloscope_mi355x_filter.hpp; src/main.cpp:103-147, Input::read in src/input.cpp:575-623):
//   teloscope <input> -o DIR [flags] [--include-bed F] [--exclude-bed F] [--include-prefix LIST] [--exclude-prefix LIST]
// A FASTA input writes DIR/<input name>_*.bed / .bedgraph / _report.tsv and the console report (scanFastaToFiles +
// printSummary); a .gfa / .gfa.gz / .gfa2 / .gfa2.gz input writes DIR/<input name>.telo.annotated.gfa and .colors.csv
// (annotateGfa).  The selection is resolved before any output file is made and before any device call.
// Test hooks:
//   --selection-only   resolve and validate the selection, print "Sequence filter: ..." on stderr and every selected record on
//                      stdout, then stop: FASTA "index<TAB>id<TAB>bases<TAB>group" per record of every group the reader makes,
//                      GFA "index<TAB>name" (no device is touched)
//   --ends-file F      GFA: the per-segment lengths come from F ("name<TAB>start<TAB>end" lines) instead of the GPU
//   --group-bytes n, --piece-bytes n, --join-lines   FASTA groups, text per host piece, records joined on the host
//   --times            "library_bases N" on stderr: the bases handed to the library
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
    std::string input, canonical, outDir = ".", endsFile;
    std::vector<std::string> rawPatterns;
    bool hasPatterns = false, manualCuration = false, readSubset = false, selectionOnly = false, times = false;
    size_t groupBytes = size_t(256) << 20, pieceBytes = size_t(4) << 20;
    int textPieces = -1;
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
            if (a == "-f") input = val();
            else if (a == "-o") outDir = val();
            else if (a == "-j") (void)val();
            else if (a == "--include-bed") addBedFilterFile(ui, val(), ui.includeBedFiles, "--include-bed");
            else if (a == "--exclude-bed") addBedFilterFile(ui, val(), ui.excludeBedFiles, "--exclude-bed");
            else if (a == "--include-prefix") addPrefixFilters(ui, val(), ui.includePrefixes, "--include-prefix");
            else if (a == "--exclude-prefix") addPrefixFilters(ui, val(), ui.excludePrefixes, "--exclude-prefix");
            else if (a == "--fastq-subset" || a == "--bam-subset") readSubset = true;
            else if (a == "--selection-only") selectionOnly = true;
            else if (a == "--ends-file") endsFile = val();
            else if (a == "--group-bytes") groupBytes = static_cast<size_t>(std::stoull(val()));
            else if (a == "--piece-bytes") pieceBytes = static_cast<size_t>(std::stoull(val()));
            else if (a == "--join-lines") textPieces = 0;
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

        if (isGfaAssemblyPath(input)) {
            if (selector.active()) validateFilteredGfa(input);
            const GfaGraph g = readGfa(input);
            const SequenceSelection sel = selectGfa(g, selector);
            if (selector.active()) std::cerr << selectionMessage(sel) << "\n";
            if (selectionOnly) {
                for (size_t k = 0; k < sel.keep.size(); ++k)
                    if (sel.keep[k]) std::cout << k << "\t" << (g.paths.empty() ? g.segments[k].name : g.paths[k].name) << "\n";
                return 0;
            }
            GfaAnnotateStats st;
            if (endsFile.empty()) {
                prepare();
                Teloscope teloscope(ui);
                st = annotateGfa(teloscope, g, &sel, outDir);
            } else {
                const std::vector<GfaEnd> jobs = gfaTerminalJobs(g, &sel.keep);
                GfaEnds e;
                e.ends.assign(g.segments.size(), {0u, 0u});
                std::ifstream in(endsFile);
                std::string seg;
                uint32_t s = 0, t = 0;
                while (in >> seg >> s >> t) {
                    const auto it = g.index.find(seg);
                    if (it != g.index.end()) e.ends[it->second] = {s, t};
                }
                for (const GfaEnd &j : jobs) if (!g.segments[j.seg].seq) ++e.noSeq;
                if (e.noSeq)
                    std::cerr << "Warning: " << e.noSeq << " of " << jobs.size()
                              << " GFA segment(s) had no sequence (*); skipped for telomere annotation.\n";
                std::filesystem::create_directories(outDir);
                const std::string stem = outDir + "/" + g.baseName + ".telo.annotated";
                st.nodes = writeAnnotatedGfa(g, jobs, e.ends, stem + ".gfa", stem + ".colors.csv");
                st.segments = g.segments.size();
                st.ends = jobs.size();
                st.noSeq = e.noSeq;
            }
            std::cout << st.segments << " " << st.ends << " " << st.scanned << " " << st.noSeq << " " << st.nodes << " "
                      << st.parseMs << " " << st.scanMs << " " << st.writeMs << "\n";
            return 0;
        }

        FastaGroupReader reader(input, groupBytes, pieceBytes, textPieces != 0, selector.active());
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
        const std::string outBase = outDir + "/" + name;
        ScanFastaTimes T;
        const AssemblySummary summary = scanFastaToFiles(teloscope, input, outBase, std::cout, manualCuration, groupBytes, &T,
                                                         pieceBytes, textPieces, &reader);
        printSummary(std::cout, summary, ui.ultraFastMode, outBase + "_report.tsv");
        if (times) std::fprintf(stderr, "library_bases %llu\n", static_cast<unsigned long long>(T.library_bases));
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
    return 0;
}
