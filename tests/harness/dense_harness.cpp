// The dense stage's per-element decision (csrc/dense_core.hpp, compiled for the host exactly as k_dense_rows compiles it) walked over
// every row shape up to `max_width` columns: n_tokens 0 .. max_width + 2 (rows that are too short and too long included -- the pipeline
// makes neither, the kernel must be safe with both), every pad count, both padding sides, 0 .. 2 special tokens in front and behind.
// A stand-alone program (tests/test_dense_core.py builds it with -fsanitize=address,undefined and runs it).  The row's arrays are heap
// blocks of EXACTLY its tokens, read through the index the routine returns, so an index outside the row is a sanitizer report; the
// program also checks it itself.  Prints one line per shape -- "n pad left n_prefix n_suffix width seq|" and per column the kind
// (T token, S special, P padding) followed by the source column or '-' -- for the test to compare with its own restatement; exits 1 on
// the first unsafe answer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense_core.hpp"

using namespace tkamd;

int main(int argc, char** argv) {
    const int64_t max_width = argc > 1 ? atoll(argv[1]) : 9;
    const int64_t a = 5;                                      // the row does not start at the array's start
    long long lines = 0;
    for (int64_t width = 1; width <= max_width; ++width)
        for (int64_t n = 0; n <= max_width + 2; ++n)
            for (uint32_t pad = 0; pad <= (uint32_t)n + 1u; ++pad)
                for (int left = 0; left < 2; ++left)
                    for (uint32_t np = 0; np < 3; ++np)
                        for (uint32_t ns = 0; ns < 3; ++ns)
                            for (int with_seq = 0; with_seq < 2; ++with_seq) {
                                // the published arrays of this row alone: ids[k] = 100 + k, and the sequence ids its layout implies
                                std::vector<uint32_t>* ids = new std::vector<uint32_t>((size_t)n);
                                std::vector<uint8_t>* seq = new std::vector<uint8_t>((size_t)(a + n), (uint8_t)3);     // (indexed by a + col, like the batch's)
                                for (int64_t k = 0; k < n; ++k) {
                                    (*ids)[(size_t)k] = 100u + (uint32_t)k;
                                    const int64_t p = pad < (uint64_t)n ? pad : n, real = n - p, r = left ? k - p : k;
                                    (*seq)[(size_t)(a + k)] = (r < 0 || r >= real) ? 3 : ((r < (int64_t)np || r >= real - (int64_t)ns) ? 2 : (uint8_t)(k & 1));
                                }
                                const uint8_t* seq_at = with_seq ? seq->data() : nullptr;
                                std::printf("%lld %u %d %u %u %lld %d|", (long long)n, pad, left, np, ns, (long long)width, with_seq);
                                const int64_t readable = dense_row_tokens(a, a + n, width);
                                if (readable != (n < width ? n : width)) { std::printf("\nFAILED: dense_row_tokens\n"); return 1; }
                                for (int64_t col = 0; col < width; ++col) {
                                    const DenseSrc s = dense_element(a, a + n, pad, left != 0, np, ns, width, col, seq_at);
                                    if (s.kind > DENSE_PAD || (s.src < 0 && s.kind != DENSE_PAD) || (s.src >= 0 && (s.src < a || s.src >= a + readable || s.src != a + col)) ||
                                        (s.src < 0) != (col >= readable)) {
                                        std::printf("\nFAILED: column %lld -> src %lld kind %u\n", (long long)col, (long long)s.src, s.kind);
                                        return 1;
                                    }
                                    if (s.src >= 0 && ids->data()[s.src - a] != 100u + (uint32_t)col) { std::printf("\nFAILED: the id read\n"); return 1; }
                                    std::printf("%c", "TSP"[s.kind]);
                                    if (s.src >= 0) std::printf("%lld", (long long)(s.src - a)); else std::printf("-");
                                    std::printf(col + 1 < width ? "," : "");
                                }
                                std::printf("\n");
                                ++lines;
                                delete ids;
                                delete seq;
                            }
    // an empty range that runs backwards reads nothing
    if (dense_row_tokens(9, 3, 4) != 0 || dense_element(9, 3, 0, false, 0, 0, 4, 0, nullptr).src != -1) { std::printf("FAILED: backwards range\n"); return 1; }
    std::printf("ok: %lld shapes\n", lines);
    return 0;
}
