// Test harness (g++, no HIP): tokenizers_amd/csrc/unigram_core.hpp -- the body the Unigram kernels run -- on the host, over the tables
// host_model.cpp builds from a tokenizer.json.  tests/test_unigram.py holds it against the reference wheel's model.tokenize; built with
// -DUNIH_MAIN it is a stand-alone program (its own main) for the sanitizer run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_model.hpp"
#include "unigram_core.hpp"

using namespace tkamd;

namespace {
struct VecState {
    struct Node { uint64_t best; uint32_t back, id; };
    std::vector<Node> n;
    void clear(uint32_t p) { n[p] = Node{0, 0, 0}; }
    bool isset(uint32_t p) const { return n[p].back != 0; }
    double score(uint32_t p) const { return uni_u2d(n[p].best); }
    uint32_t back(uint32_t p) const { return n[p].back; }
    uint32_t id(uint32_t p) const { return n[p].id; }
    void set(uint32_t p, double sc, uint32_t b, uint32_t i) { n[p] = Node{uni_d2u(sc), b, i}; }
    void set_fwd(uint32_t p, uint32_t end, uint32_t i) { n[p].best = (uint64_t)end | ((uint64_t)i << 32); }
    void get_fwd(uint32_t p, uint32_t* end, uint32_t* i) const { *end = (uint32_t)n[p].best; *i = (uint32_t)(n[p].best >> 32); }
};
struct Bytes {
    const uint8_t* p;
    uint32_t operator()(uint32_t w) const { return p[w]; }
};
struct Collect {
    std::vector<uint32_t>* ids;
    std::vector<uint32_t>* ends;
    std::vector<uint8_t>* is_byte;
    void operator()(uint32_t id, uint32_t end, bool b) { ids->push_back(id); ends->push_back(end); is_byte->push_back(b ? 1 : 0); }
};
std::unique_ptr<HostModel> g_model;
UniModel model_of(const HostModel& m) {
    UniModel u;
    u.trie = m.trie.table.data(); u.trie_mask = m.trie.mask; u.trie_seed = m.trie.seed;
    u.score = m.uni_score.data(); u.unk_score = m.uni_unk_score;
    u.unk_id = m.unk_id; u.has_unk = m.has_unk ? 1u : 0u;
    u.byte_id = m.byte_id; u.bytes_on = m.uni_bytes ? 1u : 0u;
    return u;
}
std::string g_error;
}  // namespace

extern "C" {
// 0: loaded; 1: refused / invalid (unih_error says why)
int unih_load(const char* json, size_t len) {
    try {
        g_model.reset(new HostModel(HostModel::from_json(json, len)));
        if (g_model->model != MODEL_UNIGRAM) { g_error = "not a Unigram model"; return 1; }
        return 0;
    } catch (const std::exception& e) { g_error = e.what(); return 1; }
}
const char* unih_error() { return g_error.c_str(); }
double unih_score(uint32_t id) { return g_model->uni_score[id]; }
double unih_unk_score() { return g_model->uni_unk_score; }
// words: text + CSR of n words.  Out: per word its tokens' ids / ends / byte flags, concatenated, and tok_off[n + 1]; err[w] the core's error bits.
// Returns the number of tokens, or -1 when `cap` tokens do not hold them.
int64_t unih_encode(const uint8_t* text, const int64_t* off, int64_t n, uint32_t* ids, uint32_t* ends, uint8_t* is_byte, int64_t* tok_off, uint32_t* err, int64_t cap) {
    const UniModel u = model_of(*g_model);
    std::vector<uint32_t> vi, ve;
    std::vector<uint8_t> vb;
    VecState st;
    int64_t total = 0;
    for (int64_t w = 0; w < n; ++w) {
        const uint32_t len = (uint32_t)(off[w + 1] - off[w]);
        vi.clear(); ve.clear(); vb.clear();
        st.n.assign((size_t)len + 1, VecState::Node{0, 0, 0});
        Collect c{&vi, &ve, &vb};
        const Bytes by{text + off[w]};
        err[w] = uni_encode(u, len, st, by, c);
        tok_off[w] = total;
        if (total + (int64_t)vi.size() > cap) return -1;
        memcpy(ids + total, vi.data(), vi.size() * 4);
        memcpy(ends + total, ve.data(), ve.size() * 4);
        memcpy(is_byte + total, vb.data(), vb.size());
        total += (int64_t)vi.size();
    }
    tok_off[n] = total;
    return total;
}
}

#ifdef UNIH_MAIN
// stand-alone: unigram_harness <tokenizer.json> <words file: one word a line>; prints ids and ends a word.  (The sanitizer build runs this.)
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s tokenizer.json words.txt\n", argv[0]); return 2; }
    auto slurp = [](const char* path) { std::string s; FILE* f = fopen(path, "rb"); if (!f) return s; char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, k); fclose(f); return s; };
    const std::string js = slurp(argv[1]), words = slurp(argv[2]);
    if (unih_load(js.data(), js.size())) { fprintf(stderr, "load: %s\n", unih_error()); return 1; }
    std::vector<int64_t> off{0};
    std::string text;
    for (size_t i = 0; i < words.size();) {
        size_t j = words.find('\n', i);
        if (j == std::string::npos) j = words.size();
        text.append(words, i, j - i);
        off.push_back((int64_t)text.size());
        i = j + 1;
    }
    const int64_t n = (int64_t)off.size() - 1, cap = (int64_t)text.size() + 1;
    std::vector<uint32_t> ids((size_t)cap), ends((size_t)cap), err((size_t)n + 1);
    std::vector<uint8_t> isb((size_t)cap);
    std::vector<int64_t> to((size_t)n + 1);
    // (exact-size copy of the text: a read past a word's bytes is a heap overflow the sanitizer reports)
    std::vector<uint8_t> exact(text.begin(), text.end());
    if (unih_encode(exact.data(), off.data(), n, ids.data(), ends.data(), isb.data(), to.data(), err.data(), cap) < 0) return 3;
    for (int64_t w = 0; w < n; ++w) {
        printf("%u", err[w]);
        for (int64_t k = to[w]; k < to[w + 1]; ++k) printf(" %u:%u", ids[k], ends[k]);
        printf("\n");
    }
    return 0;
}
#endif
