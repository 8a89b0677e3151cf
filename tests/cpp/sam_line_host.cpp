// sam_line_host.cpp — TEST INFRASTRUCTURE: teloscope_amd/csrc/sam_line_core.h, the per-line rule the SAM kernels compile, built for
// the host by g++ under ASan + UBSan (tests/test_sam_chunk_reference_cpu.py).  The program makes what the chunk layer hands the
// kernel — every line's start and '\r' flag, every tab's offset — by plain loops, in heap blocks of exactly the needed sizes, so
// that a read beyond the text or beyond the tab array is a sanitizer report, and calls the rule once per alignment line as the
// kernel's lanes do.
// Usage: sam_line_host FILE AT_END     a line per whole line of FILE:
//            "H <start>"                                                a header line
//            "A <start> <error> <seq_at> <seq_len> <size> <flags>"      an alignment line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/sam_line_core.h"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: sam_line_host FILE AT_END\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::string whole((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const bool at_end = std::atoi(argv[2]) != 0;
    const uint32_t n = (uint32_t)whole.size();
    unsigned char *text = (unsigned char *)std::malloc(n ? n : 1);
    std::memcpy(text, whole.data(), n);

    // the line index as chunk.hip leaves it: lstart[i + 1] is one behind line i's '\n' (n + 1 for an unfinished last line)
    std::vector<uint32_t> lstart{0};
    std::vector<unsigned char> cr;
    uint32_t n_tabs = 0;
    for (uint32_t p = 0; p < n; ++p) {
        if (text[p] == '\t') ++n_tabs;
        if (text[p] == '\n') { lstart.push_back(p + 1); cr.push_back(p > 0 && text[p - 1] == '\r'); }
    }
    if (at_end && n && text[n - 1] != '\n') { lstart.push_back(n + 1); cr.push_back(text[n - 1] == '\r'); }
    uint32_t *tabs = (uint32_t *)std::malloc(n_tabs ? n_tabs * sizeof(uint32_t) : 1);
    for (uint32_t p = 0, k = 0; p < n; ++p) if (text[p] == '\t') tabs[k++] = p;

    const uint32_t n_lines = (uint32_t)cr.size();
    for (uint32_t i = 0; i < n_lines; ++i) {
        const uint32_t ls = lstart[i], end = lstart[i + 1] - 1u - cr[i];
        if (ls < n && ls < lstart[i + 1] - 1u && text[ls] == '@') { printf("H %u\n", ls); continue; }
        tssam::Line l;
        const tssam::Error e = tssam::line_rule(text, ls, end, tabs, n_tabs, tssam::tab_lower_bound(tabs, n_tabs, ls), &l);
        printf("A %u %d %u %u %u %u\n", ls, (int)e, l.seq_at, l.seq_len, end + cr[i] - ls, l.flags);
    }
    std::free(tabs);
    std::free(text);
    return 0;
}
