// read_block_format_host.cpp — read_block_format_core.h on the host, for tests/test_read_block_format_core_cpu.py (built by g++
// with -fsanitize=address,undefined): the header the gfx950 kernels of read_blocks.hip and the host routes compile, fed from
// stdin and answered on stdout, a case per line.
//
//   L <name hex|-> <start> <block_len> <label char code> <fwd> <rev> <can> <noncan> <read_len>   ->  <line_len> <line hex>
//   F <text hex>   a FASTQ header line with its line end, and the byte behind it  ->  <name_off> <name_len>
//   S <text hex>   a SAM alignment line                                           ->  <name_off> <name_len>
//   B <text hex>   a BAM record from its block_size field on                      ->  <name_off> <name_len>
//
// The line is written into a buffer of exactly line_len bytes (a byte beyond it is ASan's to report) and every byte of it must
// have been written exactly once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/read_block_format_core.h"

namespace {

struct Bytes {
    const std::vector<unsigned char> &v;
    uint32_t byte(uint64_t i) const { return v.at(static_cast<size_t>(i)); }
};
struct Sink {
    std::vector<unsigned char> &v;
    std::vector<unsigned char> &hits;
    void put(uint32_t at, uint32_t byte) { v.at(at) = static_cast<unsigned char>(byte); ++hits.at(at); }
};

std::vector<unsigned char> unhex(const std::string &s) {
    std::vector<unsigned char> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(static_cast<unsigned char>(std::stoul(s.substr(i, 2), nullptr, 16)));
    return out;
}

void print_hex(const std::vector<unsigned char> &v) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (unsigned char c : v) { s += d[c >> 4]; s += d[c & 15]; }
    std::cout << (s.empty() ? "-" : s);
}

}  // namespace

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        std::istringstream in(row);
        std::string kind, hex;
        in >> kind >> hex;
        const std::vector<unsigned char> text = unhex(hex);
        const Bytes bytes{text};
        if (kind == "L") {
            unsigned long long start, v[7];
            in >> start;
            for (auto &x : v) in >> x;
            if (!in) { std::cerr << "bad case: " << row << "\n"; return 2; }
            const tsrb::Fields f{start, (uint32_t)v[0], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6], (uint32_t)v[1]};
            const uint32_t n = tsrb::line_len((uint32_t)text.size(), f);
            std::vector<unsigned char> line(n, 0), hits(n, 0);
            Sink s{line, hits};
            tsrb::put_line(s, 0u, bytes, 0u, (uint32_t)text.size(), f);
            for (unsigned char h : hits) if (h != 1) { std::cerr << "a byte written " << (int)h << " times: " << row << "\n"; return 3; }
            std::cout << n << " ";
            print_hex(line);
            std::cout << "\n";
        } else if (kind == "F") {
            // the header line's length with its '\n' is the record's seq_at
            size_t nl = 0;
            while (nl < text.size() && text[nl] != '\n') ++nl;
            std::cout << tsrb::fastq_name_off(0) << " " << tsrb::fastq_name_len(bytes, 0, (uint32_t)(nl + 1)) << "\n";
        } else if (kind == "S") {
            std::cout << 0 << " " << tsrb::sam_name_len(bytes, 0, (uint32_t)text.size()) << "\n";
        } else if (kind == "B") {
            std::cout << tsrb::bam_name_off(0) << " " << tsrb::bam_name_len(bytes, 0) << "\n";
        } else {
            std::cerr << "unknown case: " << row << "\n";
            return 2;
        }
    }
    return 0;
}
