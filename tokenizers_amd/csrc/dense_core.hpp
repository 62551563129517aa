// The dense stage's per-element decision (kernels/dense.hip, k_dense_rows): what column `col` of a padded [n_rows, width] row is made of.
// A row is the encoding the epilogue published -- tokens [a, z) of its CSR, padding and special tokens already in place (Encoding::pad,
// tokenizer/encoding.rs:405-470; PostProcessor::process) -- so a column either names one source index of that CSR or lies beyond it, and
// is one of three kinds: a token of the text, a special token, padding.  The kind comes from the sequence ids where the epilogue wrote
// them (pairs, typed single templates: 0 / 1 sequence A / B, 2 special, 3 padding), else from the row's pad count, the padding side and
// the number of special tokens in front of / behind the sequence -- the layout of Encoding._layout in tokenizers_amd/tokenizer.py.
// One host+device function, so that the CPU test runs exactly what the kernel runs (tests/harness/dense_harness.cpp).
#pragma once
#include <cstdint>

#include "tables.hpp"

namespace tkamd {

enum : uint32_t { DENSE_TOKEN = 0, DENSE_SPECIAL = 1, DENSE_PAD = 2 };

struct DenseSrc {
    int64_t src;        // index into the published per-token arrays, or -1: the column lies beyond the row's tokens (written as padding)
    uint32_t kind;      // DENSE_TOKEN / DENSE_SPECIAL / DENSE_PAD
};

// Tokens of the row a dense row of `width` columns may read: z - a, never more than width, 0 for a range that runs backwards.
TK_HD int64_t dense_row_tokens(int64_t a, int64_t z, int64_t width) {
    const int64_t n = z - a;
    return n < 0 ? 0 : (n > width ? width : n);
}

// Column col (0 <= col < width) of the row [a, z) with `pads` padding tokens on the left (pad_left) or right, n_prefix / n_suffix special
// tokens around the sequence; seq_ids: the published sequence ids or null.  A row of exactly width tokens is the only one the pipeline
// makes (tkamd_dense_width); any other is still read inside [a, z) only, and the columns it does not reach come out as padding.
TK_HD DenseSrc dense_element(int64_t a, int64_t z, uint32_t pads, bool pad_left, uint32_t n_prefix, uint32_t n_suffix, int64_t width, int64_t col,
                             const uint8_t* seq_ids) {
    const int64_t n = dense_row_tokens(a, z, width);
    if (col >= n) return DenseSrc{-1, DENSE_PAD};
    const int64_t src = a + col;
    if (seq_ids) {
        const uint32_t q = seq_ids[src];
        return DenseSrc{src, q >= 3u ? DENSE_PAD : (q == 2u ? DENSE_SPECIAL : DENSE_TOKEN)};
    }
    const int64_t p = (int64_t)pads < n ? (int64_t)pads : n;      // (a pad count beyond the row: the whole row is padding)
    const int64_t real = n - p;                                   // prefix + sequence + suffix
    const int64_t r = pad_left ? col - p : col;                   // position inside them
    if (r < 0 || r >= real) return DenseSrc{src, DENSE_PAD};
    if (r < (int64_t)n_prefix || r >= real - (int64_t)n_suffix) return DenseSrc{src, DENSE_SPECIAL};
    return DenseSrc{src, DENSE_TOKEN};
}

}  // namespace tkamd
