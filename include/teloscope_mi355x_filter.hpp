// teloscope_mi355x_filter.hpp — assembly record filters (--include-bed / --exclude-bed / --include-prefix / --exclude-prefix;
// reference: src/main.cpp:103-147, SequenceSelector in src/input.cpp:384-563, docs/parameters.md "Assembly record filters").
// Header-only; the selection itself is host work.  It decides which FASTA records / GFA paths / GFA segments reach the scan.  On
// the host routes (scanFastaToFiles with a selected FastaGroupReader, annotateGfa) the device never sees the others; on the
// device routes (scanFastaToFilesDevice and annotateGfaDevice with a selector) their text lies in device memory with the rest,
// is checked there by the filtered loaders' rules (ts_fasta_chunk_strict, ts_gfa_chunk_check) and is never joined or scanned.
//
//     addPrefixFilters(ui, "hap1_chr,hap2_chr", ui.includePrefixes, "--include-prefix");   // option parsing
//     addBedFilterFile(ui, "primary.ids", ui.includeBedFiles, "--include-bed");
//     SequenceSelector selector(ui);                                   // reads the selector files
//     SequenceSelection sel = selector.select(names, "paths");         // keep flags, in the order of `names`
//
// Every error the reference answers with "Error: <message>" and exit(EXIT_FAILURE) is thrown as a SequenceFilterError carrying
// the same message; the library never exits.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "teloscope_mi355x.hpp"

namespace teloscope_mi355x {

struct SequenceFilterError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// what SequenceSelector::select decided: keep[i] for candidate i, and the counts the reports print
struct SequenceSelection {
    std::vector<char> keep;
    uint64_t inputCount = 0, selectedCount = 0;
    std::string domain;                        // "paths" or "segments"
};

namespace detail {

inline std::string trimFilterText(const std::string &v) {
    const size_t a = v.find_first_not_of(" \t\r\n");
    if (a == std::string::npos) return std::string();
    return v.substr(a, v.find_last_not_of(" \t\r\n") - a + 1);
}

inline bool startsWith(const std::string &v, const std::string &prefix) {
    return v.size() >= prefix.size() && v.compare(0, prefix.size(), prefix) == 0;
}

inline bool caseInsensitiveSuffix(const std::string &v, const std::string &sfx) {
    if (v.size() < sfx.size()) return false;
    for (size_t i = 0; i < sfx.size(); ++i) {
        const unsigned char a = static_cast<unsigned char>(v[v.size() - sfx.size() + i]), b = static_cast<unsigned char>(sfx[i]);
        if (std::tolower(a) != std::tolower(b)) return false;
    }
    return true;
}

// a BED coordinate: digits only, fits in 64 bits
inline bool parseCoordinate(const std::string &v, uint64_t &out) {
    if (v.empty()) return false;
    uint64_t x = 0;
    for (char c : v) {
        if (c < '0' || c > '9') return false;
        const uint64_t d = static_cast<uint64_t>(c - '0');
        if (x > (UINT64_MAX - d) / 10) return false;
        x = x * 10 + d;
    }
    out = x;
    return true;
}

// 'a', 'b', ... (and N more): at most ten names
inline std::string describeNames(const std::vector<std::string> &v) {
    std::string s;
    const size_t shown = std::min<size_t>(v.size(), 10);
    for (size_t i = 0; i < shown; ++i) s += (i ? ", '" : "'") + v[i] + "'";
    if (v.size() > shown) s += " (and " + std::to_string(v.size() - shown) + " more)";
    return s;
}

inline std::vector<std::string> sortedUnique(std::vector<std::string> v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

}  // namespace detail

// The name a filter compares: a header up to its first whitespace (space, tab, CR, LF, FF, VT)
inline std::string sequenceFilterId(const std::string &header) {
    return header.substr(0, header.find_first_of(" \t\r\n\f\v"));
}

// GFA mode is chosen by the input's name: .gfa, .gfa.gz, .gfa2, .gfa2.gz in any letter case
inline bool isGfaAssemblyPath(const std::string &path) {
    return detail::caseInsensitiveSuffix(path, ".gfa") || detail::caseInsensitiveSuffix(path, ".gfa.gz") ||
           detail::caseInsensitiveSuffix(path, ".gfa2") || detail::caseInsensitiveSuffix(path, ".gfa2.gz");
}

// --include-bed / --exclude-bed FILE: the file must exist and be a regular file; its resolved path is appended to `files`
inline void addBedFilterFile(UserInputTeloscope &ui, const std::string &path, std::vector<std::string> &files, const char *optionName) {
    namespace fs = std::filesystem;
    std::error_code ec;
    const fs::path p(path);
    if (path.empty() || !fs::exists(p, ec) || ec)
        throw SequenceFilterError(std::string(optionName) + " file does not exist: '" + path + "'.");
    if (!fs::is_regular_file(p, ec) || ec)
        throw SequenceFilterError(std::string(optionName) + " file '" + path + "' is not a regular file.");
    const fs::path resolved = fs::canonical(p, ec);
    if (ec) throw SequenceFilterError(std::string("Could not resolve ") + optionName + " file '" + path + "': " + ec.message() + ".");
    files.push_back(resolved.string());
    ui.sequenceFilterActive = true;
}

// --include-prefix / --exclude-prefix LIST: comma-separated, each prefix trimmed of space, tab, CR and LF; an empty value, an
// empty prefix or a trailing comma is an error
inline void addPrefixFilters(UserInputTeloscope &ui, const std::string &value, std::vector<std::string> &prefixes, const char *optionName) {
    const std::string empty = std::string(optionName) + " contains an empty prefix.";
    if (value.empty() || value.back() == ',') throw SequenceFilterError(empty);
    std::istringstream in(value);
    for (std::string tok; std::getline(in, tok, ',');) {
        tok = detail::trimFilterText(tok);
        if (tok.empty()) throw SequenceFilterError(empty);
        prefixes.push_back(tok);
    }
    ui.sequenceFilterActive = true;
}

class SequenceSelector {
    std::unordered_set<std::string> includeIds, excludeIds;
    std::vector<std::string> includePrefixes, excludePrefixes;
    bool on = false;

    static std::vector<std::string> unique(const std::vector<std::string> &v) {
        std::unordered_set<std::string> seen;
        std::vector<std::string> out;
        for (const std::string &s : v)
            if (seen.insert(s).second) out.push_back(s);
        return out;
    }

    // one ID per line, or BED3+ rows (the coordinates are checked, never applied); blank, '#', track and browser lines skipped
    static void load(const std::vector<std::string> &files, std::unordered_set<std::string> &ids, const char *optionName) {
        for (const std::string &path : files) {
            std::ifstream in(path, std::ios::binary);
            if (!in) throw SequenceFilterError(std::string("Could not open ") + optionName + " file '" + path + "'.");
            uint64_t lineNo = 0, idLines = 0;
            for (std::string raw; std::getline(in, raw);) {
                ++lineNo;
                if (lineNo == 1 && raw.size() >= 3 && static_cast<unsigned char>(raw[0]) == 0xef &&
                    static_cast<unsigned char>(raw[1]) == 0xbb && static_cast<unsigned char>(raw[2]) == 0xbf)
                    raw.erase(0, 3);
                const std::string line = detail::trimFilterText(raw);
                if (line.empty() || line[0] == '#') continue;
                std::istringstream fs(line);
                std::vector<std::string> f;
                for (std::string x; fs >> x;) f.push_back(x);
                if (f.empty() || f[0] == "track" || f[0] == "browser") continue;
                const std::string at = path + ":" + std::to_string(lineNo);
                if (f.size() == 2) throw SequenceFilterError(at + " must contain either one ID column or at least three BED columns.");
                uint64_t b = 0, e = 0;
                if (f.size() >= 3 && !(detail::parseCoordinate(f[1], b) && detail::parseCoordinate(f[2], e) && b <= e))
                    throw SequenceFilterError(at + " has invalid BED start/end coordinates.");
                ids.insert(f[0]);
                ++idLines;
            }
            if (!idLines) throw SequenceFilterError(std::string(optionName) + " file '" + path + "' contains no sequence IDs.");
        }
    }

    static bool anyPrefix(const std::string &name, const std::vector<std::string> &prefixes) {
        for (const std::string &p : prefixes)
            if (detail::startsWith(name, p)) return true;
        return false;
    }

public:
    explicit SequenceSelector(const UserInputTeloscope &ui)
        : includePrefixes(unique(ui.includePrefixes)), excludePrefixes(unique(ui.excludePrefixes)), on(ui.sequenceFilterActive) {
        load(ui.includeBedFiles, includeIds, "--include-bed");
        load(ui.excludeBedFiles, excludeIds, "--exclude-bed");
    }

    bool active() const { return on; }

    // included = no include selector, or an include ID / prefix matches; excluded = an exclude ID / prefix matches.  When
    // filtering is on, the candidates and the selectors are validated first (empty or duplicate names, IDs and prefixes that
    // match nothing, an empty result).  domain: "paths" or "segments", as the messages say.
    SequenceSelection select(const std::vector<std::string> &names, const std::string &domain) const {
        SequenceSelection sel;
        sel.domain = domain;
        sel.inputCount = names.size();
        if (on) {
            std::unordered_set<std::string> seen;
            std::vector<std::string> dups;
            for (const std::string &n : names) {
                if (n.empty()) throw SequenceFilterError("Input contains an empty primary sequence ID.");
                if (!seen.insert(n).second) dups.push_back(n);
            }
            if (!dups.empty())
                throw SequenceFilterError("Input contains duplicate primary sequence ID(s): " +
                                          detail::describeNames(detail::sortedUnique(dups)) + ".");
            std::vector<std::string> idMiss, prefixMiss;
            for (const auto *ids : {&includeIds, &excludeIds})
                for (const std::string &id : *ids)
                    if (!seen.count(id)) idMiss.push_back(id);
            for (const auto *ps : {&includePrefixes, &excludePrefixes})
                for (const std::string &p : *ps)
                    if (std::none_of(names.begin(), names.end(), [&](const std::string &n) { return detail::startsWith(n, p); }))
                        prefixMiss.push_back(p);
            if (!idMiss.empty())
                throw SequenceFilterError("Sequence filter ID(s) matched no input " + domain + ": " +
                                          detail::describeNames(detail::sortedUnique(idMiss)) + ".");
            if (!prefixMiss.empty())
                throw SequenceFilterError("Sequence filter prefix(es) matched no input " + domain + ": " +
                                          detail::describeNames(detail::sortedUnique(prefixMiss)) + ".");
        }
        const bool hasIncludes = !includeIds.empty() || !includePrefixes.empty();
        sel.keep.resize(names.size());
        for (size_t i = 0; i < names.size(); ++i) {
            const std::string &n = names[i];
            const bool included = !hasIncludes || includeIds.count(n) || anyPrefix(n, includePrefixes);
            const bool excluded = excludeIds.count(n) || anyPrefix(n, excludePrefixes);
            sel.keep[i] = included && !excluded;
            sel.selectedCount += sel.keep[i] ? 1 : 0;
        }
        if (on && sel.selectedCount == 0) throw SequenceFilterError("Sequence filters excluded all input " + domain + ".");
        return sel;
    }
};

// the line the reference prints on stderr once the selection is made
inline std::string selectionMessage(const SequenceSelection &s) {
    return "Sequence filter: selected " + std::to_string(s.selectedCount) + " of " + std::to_string(s.inputCount) + " " + s.domain + ".";
}

}  // namespace teloscope_mi355x
