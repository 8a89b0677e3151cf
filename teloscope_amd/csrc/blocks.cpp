// blocks.cpp — host helpers of block calling and of the window metrics (C++17).
//
// Product restatement of Teloscope::labelTerminalBlocks (src/teloscope.cpp:259-383) and the float window
// metrics (include/teloscope.h:199-214).  The blocks themselves are called on the device (blockcall.hip).
#include "host.hpp"

#include <algorithm>
#include <cmath>

namespace ts {

int label_terminal_blocks(ts_block *blocks, size_t n, uint16_t gaps, uint64_t path_size,
                          uint32_t terminal_limit, std::string &label) {
    const int g = gaps > 0 ? 1 : 0;
    label.clear();
    for (size_t i = 0; i < n; ++i) blocks[i].is_longest = 0;
    if (n == 0) return TS_NONE + g;

    std::sort(blocks, blocks + n, [](const ts_block &a, const ts_block &b) { return a.start < b.start; });

    std::vector<ts_block *> ends;                    // scaffold-terminal blocks
    for (size_t i = 0; i < n; ++i) {
        const uint64_t bend = blocks[i].start + blocks[i].block_len;
        if (blocks[i].start < terminal_limit || bend > path_size - static_cast<uint64_t>(terminal_limit))
            ends.push_back(&blocks[i]);
    }
    std::vector<size_t> label_pos(n);
    for (size_t i = 0; i < n; ++i) {
        label_pos[i] = label.size();
        label.push_back(blocks[i].block_label);
        if (!blocks[i].has_valid_or) label.push_back('*');
    }

    ts_block *best_p = nullptr, *best_q = nullptr;
    uint64_t cov_p = 0, cov_q = 0;
    for (ts_block *b : ends) {
        if (b->block_label == 'p' && b->can_covered > cov_p) { best_p = b; cov_p = b->can_covered; }
        else if (b->block_label == 'q' && b->can_covered > cov_q) { best_q = b; cov_q = b->can_covered; }
    }
    if (best_p) best_p->is_longest = 1;
    if (best_q) best_q->is_longest = 1;
    for (size_t i = 0; i < n; ++i)
        if (blocks[i].is_longest)
            label[label_pos[i]] = static_cast<char>(std::toupper(static_cast<unsigned char>(label[label_pos[i]])));

    if ((best_p && !best_p->has_valid_or) || (best_q && !best_q->has_valid_or)) return TS_DISCORDANT + g;
    if (best_p && best_q) return (best_p->start < best_q->start ? TS_T2T : TS_MISASSEMBLY) + g;
    if (best_p)
        for (const ts_block *b : ends)
            if (b->block_label == 'p' && b != best_p && b->has_valid_or) return TS_MISASSEMBLY + g;
    if (best_q)
        for (const ts_block *b : ends)
            if (b->block_label == 'q' && b != best_q && b->has_valid_or) return TS_MISASSEMBLY + g;
    if (!best_p && !best_q) return TS_NONE + g;
    return TS_INCOMPLETE + g;
}

// getGCContent: float division, double multiply, narrowed (include/teloscope.h:211-214)
float gc_content(const uint32_t counts[4], uint32_t window_size) {
    const uint32_t gc = counts[1] + counts[2];
    return static_cast<float>(gc) / window_size * 100.0;
}

// getShannonEntropy: float32 throughout, rounded to 3 decimals (include/teloscope.h:199-208)
float shannon_entropy(const uint32_t counts[4], uint32_t window_size) {
    float entropy = 0.0;
    for (int i = 0; i < 4; ++i) {
        if (counts[i] > 0) {
            const float p = static_cast<float>(counts[i]) / window_size;
            entropy -= p * std::log2(p);
        }
    }
    return std::round(entropy * 1000.0f) / 1000.0f;
}

// The same with the four terms p log2 p looked up: a count c of a window of `w` bases always gives the same term, and a
// scan converts millions of windows of one size (log2f four times per window was most of the host's share of a scan
// without match vectors).  term[c] is computed by the expression above, so the sum is the same float.
void entropy_terms(uint32_t w, std::vector<float> &term) {
    term.assign((size_t)w + 1, 0.0f);
    for (uint32_t c = 1; c <= w; ++c) {
        const float p = static_cast<float>(c) / w;
        term[c] = p * std::log2(p);
    }
}

float shannon_entropy_memo(const uint32_t counts[4], uint32_t window_size, const std::vector<float> &term) {
    if (term.size() != (size_t)window_size + 1) return shannon_entropy(counts, window_size);
    float entropy = 0.0;
    for (int i = 0; i < 4; ++i) {
        if (counts[i] > 0) {
            if (counts[i] > window_size) return shannon_entropy(counts, window_size);
            entropy -= term[counts[i]];
        }
    }
    return std::round(entropy * 1000.0f) / 1000.0f;
}

}  // namespace ts
