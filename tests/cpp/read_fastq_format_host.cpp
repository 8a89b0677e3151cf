// read_fastq_format_host.cpp — read_fastq_format_core.h on the host, for tests/test_read_fastq_format_core_cpu.py (built by g++
// with -fsanitize=address,undefined): the header the gfx950 kernels of read_fastq.hip and the host routes compile, fed from a
// file of cases (or stdin) and answered on stdout, a case per line.
//
//   B <flags> <record hex>   a BAM record from its block_size field on        ->  <record_len> <text hex>
//   S <flags> <line hex>     a SAM alignment line without its '\n' (a trailing '\r' included)
//                                                                              ->  <record_len> <text hex>
//   read_fastq_format_host --constants                                         ->  "piece_bytes <n>"
//
// flags: 0 or 1 (TS_FASTQ_OUT_RESTORE_STRAND).  The record's bytes are held in a buffer of exactly their size and read through
// at(): a byte beyond them is an exception, and ASan's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/read_fastq_format_core.h"

namespace {

struct Bytes {
    const std::vector<unsigned char> &v;
    uint32_t byte(uint64_t i) const { return v.at(static_cast<size_t>(i)); }
};

std::vector<unsigned char> unhex(const std::string &s) {
    std::vector<unsigned char> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(static_cast<unsigned char>(std::stoul(s.substr(i, 2), nullptr, 16)));
    return out;
}

uint32_t le32(const std::vector<unsigned char> &v, size_t at) {
    return (uint32_t)v.at(at) | (uint32_t)v.at(at + 1) << 8 | (uint32_t)v.at(at + 2) << 16 | (uint32_t)v.at(at + 3) << 24;
}

void print_text(const Bytes &bytes, const tsfq::Rec &r) {
    static const char *d = "0123456789abcdef";
    const uint64_t n = tsfq::record_len(r);
    std::string s;
    for (uint64_t k = 0; k < n; ++k) { const uint32_t c = tsfq::out_byte(bytes, r, k); s += d[(c >> 4) & 15]; s += d[c & 15]; }
    std::cout << n << " " << s << "\n";
}

int run(std::istream &cases) {
    std::string row;
    while (std::getline(cases, row)) {
        std::istringstream in(row);
        std::string kind, hex;
        unsigned flags = 0;
        in >> kind >> flags >> hex;
        if (!in) { std::cerr << "bad case: " << row << "\n"; return 2; }
        const std::vector<unsigned char> text = unhex(hex);
        const Bytes bytes{text};
        if (kind == "B") {
            const uint32_t block_size = le32(text, 0), l_read_name = text.at(12), n_cigar = text.at(16) | text.at(17) << 8, l_seq = le32(text, 20);
            print_text(bytes, tsfq::bam_locate(bytes, 0, block_size, 36u + l_read_name + 4u * n_cigar, l_seq, flags));
        } else if (kind == "S") {
            // SEQ lies between tabs 9 and 10, as the walk's table says
            size_t tabs = 0, seq_at = 0, seq_end = 0;
            for (size_t i = 0; i < text.size() && tabs < 10; ++i)
                if (text[i] == '\t') { ++tabs; if (tabs == 9) seq_at = i + 1; if (tabs == 10) seq_end = i; }
            if (tabs < 10) { std::cerr << "fewer than 11 fields: " << row << "\n"; return 2; }
            print_text(bytes, tsfq::sam_locate(bytes, 0, (uint32_t)seq_at, (uint32_t)(seq_end - seq_at), (uint32_t)text.size(), flags));
        } else {
            std::cerr << "unknown case: " << row << "\n";
            return 2;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "--constants") {
        std::cout << "piece_bytes " << tsfq::kPieceBytes << "\n";
        return 0;
    }
    if (argc > 1) {
        std::ifstream file(argv[1]);
        if (!file) { std::cerr << "cannot open " << argv[1] << "\n"; return 2; }
        return run(file);
    }
    return run(std::cin);
}
