// Stand-alone driver of csrc/hot_table_core.hpp for tests/test_hot_table_core.py (built with -fsanitize=address,undefined, no HIP).
//   hot_table_harness core   < words     the builder: its table, what it placed
//   hot_table_harness parent < words     the rule the table was built by before it had weights, written out on its own: the lowest ids,
//                                        a bucket nothing fits loses its highest id (weights ignored)
// words: "slots seed n" and n lines "k0 k1 k2 len id weight" (decimal).  Output: "n_hot N", "weight W", "blob HEX", "placed i j ...".
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tokenizers_amd/csrc/hot_table_core.hpp"

using namespace tkamd;

static HotTableBuild parent_rule(const std::vector<HotWord>& words, uint32_t slots, uint32_t seed) {
    HotTableBuild out;
    const uint32_t n_buckets = slots / 4u;
    std::vector<HotSlot> hot(slots, HotSlot{0u, 0u, 0u, 0u});
    std::vector<uint16_t> disp(n_buckets, 0);
    std::vector<uint32_t> cand;
    for (uint32_t i = 0; i < (uint32_t)words.size(); ++i) cand.push_back(i);
    std::sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return words[a].id < words[b].id; });
    if (cand.size() > (size_t)slots * 15 / 16) cand.resize((size_t)slots * 15 / 16);
    auto hash_of = [&](uint32_t i) { return hot_hash(words[i].k0, words[i].k1, words[i].k2, words[i].len, seed); };
    std::vector<std::vector<uint32_t>> buckets(n_buckets);
    for (uint32_t i : cand) buckets[hot_bucket(hash_of(i), slots)].push_back(i);
    std::vector<uint32_t> order(n_buckets);
    for (uint32_t i = 0; i < n_buckets; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return buckets[a].size() > buckets[b].size(); });
    for (uint32_t bi : order) {
        std::vector<uint32_t>& bk = buckets[bi];
        while (!bk.empty()) {
            uint32_t d = 0;
            for (; d < slots; ++d) {
                bool ok = true;
                for (size_t i = 0; i < bk.size() && ok; ++i) {
                    const uint32_t s = hot_slot(hash_of(bk[i]), d, slots);
                    ok = hot[s].id_len == 0u;
                    for (size_t j = 0; j < i && ok; ++j) ok = hot_slot(hash_of(bk[j]), d, slots) != s;
                }
                if (ok) break;
            }
            if (d < slots) {
                disp[bi] = (uint16_t)d;
                for (uint32_t i : bk) {
                    hot[hot_slot(hash_of(i), d, slots)] = HotSlot{words[i].k0, words[i].k1, words[i].k2, words[i].id | (words[i].len << 24)};
                    out.placed.push_back(i);
                    out.weight_placed += words[i].weight;
                }
                out.n_hot += (int)bk.size();
                break;
            }
            bk.pop_back();
        }
    }
    out.blob.assign((size_t)hot_table_bytes((int)slots), 0);
    memcpy(out.blob.data(), hot.data(), (size_t)slots * 16);
    memcpy(out.blob.data() + (size_t)slots * 16, disp.data(), (size_t)n_buckets * 2);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 2 || (strcmp(argv[1], "core") && strcmp(argv[1], "parent"))) { fprintf(stderr, "usage: hot_table_harness core|parent < words\n"); return 2; }
    uint32_t slots = 0, seed = 0;
    size_t n = 0;
    if (scanf("%" SCNu32 " %" SCNu32 " %zu", &slots, &seed, &n) != 3 || slots < 16 || (slots & (slots - 1)) || slots > 65536) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<HotWord> words(n);
    for (HotWord& w : words)
        if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64, &w.k0, &w.k1, &w.k2, &w.len, &w.id, &w.weight) != 6) { fprintf(stderr, "bad word\n"); return 2; }
    const HotTableBuild b = strcmp(argv[1], "core") ? parent_rule(words, slots, seed) : build_hot_table_core(words, slots, seed);
    printf("n_hot %d\nweight %" PRIu64 "\nblob ", b.n_hot, b.weight_placed);
    for (uint8_t c : b.blob) printf("%02x", c);
    printf("\nplaced");
    for (uint32_t i : b.placed) printf(" %u", i);
    printf("\n");
    return 0;
}
