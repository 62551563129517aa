// The hot-word table's builder (tables.hpp has the layout): which settled words of <= 12 bytes it holds, and where.  Plain C++, no HIP:
// capi/tables.cpp builds the load-time table and every later one with it, tests/harness/hot_table_harness.cpp drives it alone.
//
// The words come with a WEIGHT -- how often each stood as a whole pre-token in the text the handle has seen (the census of
// kernels/lookup.hip k_hot_census; all equal before a census has run).  The table takes the heaviest words that fit at 15/16 full, ties to
// the lower id: with equal weights that is the lowest ids, what the table held before it learned anything -- trainers hand out ids in
// frequency order, which holds for tokens and not for whole pre-tokens (the low ids of a byte-level BPE are fragments, "he", "in", "re").
// Any subset of the eligible words is a valid table: a word that is not in it is answered by the short-word table behind it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "tables.hpp"

namespace tkamd {

struct HotWord {
    uint32_t k0, k1, k2;     // the key bytes, zero padded
    uint32_t len;            // 1 .. HOT_MAX_KEY
    uint32_t id;
    uint64_t weight;
};

struct HotTableBuild {
    std::vector<uint8_t> blob;        // hot_table_bytes(slots): the slots, then the displacements
    std::vector<uint32_t> placed;     // indices into the words given, in no particular order
    int n_hot = 0;
    uint64_t weight_placed = 0;       // the sum of the placed words' weights
};

// Hash-and-displace: the fullest buckets first, each takes the first displacement that drops all of its words on free slots; a bucket
// nothing fits loses its lightest word (ties: the highest id) and tries again.
inline HotTableBuild build_hot_table_core(const std::vector<HotWord>& words, uint32_t slots, uint32_t seed) {
    HotTableBuild out;
    const uint32_t n_buckets = slots / 4u;
    std::vector<HotSlot> hot(slots, HotSlot{0u, 0u, 0u, 0u});
    std::vector<uint16_t> disp(n_buckets, 0);
    std::vector<uint32_t> cand;
    for (uint32_t i = 0; i < (uint32_t)words.size(); ++i)
        if (words[i].len && words[i].len <= (uint32_t)HOT_MAX_KEY) cand.push_back(i);
    // the heaviest words, ties to the lower id (then the key, so that the order never depends on the order given), as many as fit at 15/16 full
    std::sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) {
        const HotWord &a = words[x], &b = words[y];
        if (a.weight != b.weight) return a.weight > b.weight;
        if (a.id != b.id) return a.id < b.id;
        if (a.len != b.len) return a.len < b.len;
        if (a.k0 != b.k0) return a.k0 < b.k0;
        if (a.k1 != b.k1) return a.k1 < b.k1;
        return a.k2 < b.k2;
    });
    if (cand.size() > (size_t)slots * 15 / 16) cand.resize((size_t)slots * 15 / 16);
    auto hash_of = [&](uint32_t i) { return hot_hash(words[i].k0, words[i].k1, words[i].k2, words[i].len, seed); };
    std::vector<std::vector<uint32_t>> buckets(n_buckets);
    for (uint32_t i : cand) buckets[hot_bucket(hash_of(i), slots)].push_back(i);      // (heaviest first inside a bucket)
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
                    const HotWord& w = words[i];
                    hot[hot_slot(hash_of(i), d, slots)] = HotSlot{w.k0, w.k1, w.k2, w.id | (w.len << 24)};
                    out.placed.push_back(i);
                    out.weight_placed += w.weight;
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

}  // namespace tkamd
