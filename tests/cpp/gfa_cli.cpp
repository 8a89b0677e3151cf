// gfa_cli.cpp — TEST INFRASTRUCTURE: a C++17 driver of the GFA front end (include/teloscope_mi355x_gfa.hpp), so that the
// reference's GFA manifests (validateFiles/gfa*.tst) can be replayed through it: `teloscope asm.gfa -o out/` writes
// out/asm.gfa.telo.annotated.gfa and out/asm.gfa.telo.annotated.colors.csv (src/input.cpp:625-716).
// Usage: gfa_cli <flags as in the manifest's first line, input path already resolved>
//        [--ends-file F]   test hook: the per-segment lengths come from F ("name<TAB>start<TAB>end" lines) instead of the
//                          GPU — the host logic (parse, ends, write) runs on a machine without one
// Prints "segments ends scanned no_seq nodes parse_ms scan_ms write_ms" on stdout; errors go to stderr with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_gfa.hpp"

using namespace teloscope_mi355x;

int main(int argc, char **argv) {
    UserInputTeloscope ui;
    std::string input, canonical, outDir = ".", endsFile;
    std::vector<std::string> rawPatterns;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) exit(EXIT_FAILURE); return argv[++i]; };
        if (a == "-f") input = val();
        else if (a == "-o") outDir = val();
        else if (a == "-j") (void)val();
        else if (a == "--ends-file") endsFile = val();
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
    try {
        GfaAnnotateStats st;
        if (endsFile.empty()) {
            if (!canonical.empty()) setCanonical(ui, canonical);
            ui.rawPatterns = rawPatterns.empty() ? std::vector<std::string>{ui.canonicalFwd, ui.canonicalRev} : rawPatterns;
            ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
            Teloscope teloscope(ui);
            st = annotateGfa(teloscope, input, outDir);
        } else {
            const GfaGraph g = readGfa(input);
            const std::vector<GfaEnd> jobs = gfaTerminalJobs(g);
            GfaEnds e;
            e.ends.assign(g.segments.size(), {0u, 0u});
            std::ifstream in(endsFile);
            std::string name;
            uint32_t s = 0, t = 0;
            while (in >> name >> s >> t) {
                const auto it = g.index.find(name);
                if (it != g.index.end()) e.ends[it->second] = {s, t};
            }
            for (const GfaEnd &j : jobs) if (!g.segments[j.seg].seq) ++e.noSeq;
            if (e.noSeq)
                std::cerr << "Warning: " << e.noSeq << " of " << jobs.size()
                          << " GFA segment(s) had no sequence (*); skipped for telomere annotation.\n";
            const std::string stem = outDir + "/" + g.baseName + ".telo.annotated";
            st.nodes = writeAnnotatedGfa(g, jobs, e.ends, stem + ".gfa", stem + ".colors.csv");
            st.segments = g.segments.size();
            st.ends = jobs.size();
            st.noSeq = e.noSeq;
        }
        std::cout << st.segments << " " << st.ends << " " << st.scanned << " " << st.noSeq << " " << st.nodes << " "
                  << st.parseMs << " " << st.scanMs << " " << st.writeMs << "\n";
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
}
