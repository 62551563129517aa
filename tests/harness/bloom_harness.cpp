// CPU harness for tokenizers_amd/csrc/pretok_bloom_core.hpp: computes the start mask and the lead mask of a batch the way
// k_pretok_bloom does -- one "lane" per 64-byte mask word, 256 lanes a workgroup, the packed `up` / `down` words handed between
// neighbouring lanes, bloom_edge_up / bloom_edge_down at the workgroup's two ends -- with the tables of the tokenizer.json it is given
// (which must load as PT_BLOOM).  Built as a shared library by tests/test_bloom.py (g++, no GPU), and as a stand-alone program
// (-DBLOOM_STANDALONE, with -fsanitize=address,undefined) that reads the same inputs from files.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_model.hpp"
#include "pretok_bloom_core.hpp"

using namespace tkamd;

namespace {
constexpr int64_t WG = 256;      // the kernel's workgroup: one lane a word

struct Text {
    std::vector<uint8_t> buf;    // garbage in front, the text (16-byte aligned, as the device's is), then the 64 readable bytes of TKAMD_TEXT_PAD (garbage
    uint8_t* t;                  // too) and at most 15 more: a read further out is one the sanitizer build reports
    Text(const uint8_t* text, int64_t n) : buf((size_t)n + 64 + 15 + 64, 0xEE) {
        t = buf.data() + 64;
        t += (16 - ((uintptr_t)t & 15)) & 15;
        if (n) memcpy(t, text, (size_t)n);
    }
};

void run(const HostModel& hm, const uint8_t* t, int64_t n, const std::vector<uint64_t>& docmask, int64_t n_words, uint64_t* start, uint64_t* lead) {
    uint32_t lut[256];
    for (uint32_t v = 0; v < 256; ++v) lut[v] = bloom_byte_flags(v);
    const uint16_t* uc1 = hm.uc_stage1.data();
    const uint8_t* uc2 = hm.uc_stage2.data();
    const int64_t n_blocks = (n_words + WG - 1) / WG;
    std::vector<BloomWord> m((size_t)WG);
    std::vector<uint32_t> up((size_t)WG), down((size_t)WG);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t w0 = b * WG;
        for (int64_t i = 0; i < WG; ++i) {
            bloom_word_classify(t, n, docmask.data(), lut, w0 + i, uc1, uc2, m[i]);
            up[i] = bloom_pack_up(m[i]);
            down[i] = bloom_pack_down(m[i]);
        }
        // the two ends of the workgroup: threads 0 and 1 of the kernel
        const int64_t front = w0 << 6, behind = (w0 + WG) << 6;
        const uint32_t edge_up = (w0 > 0 && front < n) ? bloom_edge_up(t, front, lut, uc1, uc2) : 0u;
        const uint32_t edge_down = behind < n ? bloom_edge_down(t, behind, docmask.data(), lut, uc1, uc2) : 0u;
        for (int64_t i = 0; i < WG; ++i) {
            const int64_t w = w0 + i;
            uint64_t ld = 0;
            const uint64_t out = bloom_word_starts(m[i], i == 0 ? edge_up : up[i - 1], i == WG - 1 ? edge_down : down[i + 1], w, n, &ld);
            if (w < n_words) { start[w] = out; lead[w] = ld; }
        }
    }
}
}  // namespace

// start / lead: (n >> 6) + 1 words each.  -1: the file does not load as PT_BLOOM
extern "C" int blh_run(const char* json, size_t json_len, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs, uint64_t* start, uint64_t* lead) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    if (hm.pretok != PT_BLOOM) return -1;
    const int64_t n_words = (n >> 6) + 1;
    std::vector<uint64_t> docmask((size_t)n_words + 1, 0);
    for (int64_t d = 0; d < n_docs; ++d)
        if (doc_off[d] < n) docmask[doc_off[d] >> 6] |= 1ull << (doc_off[d] & 63);
    Text tx(text, n);
    for (int64_t w = 0; w < n_words; ++w) start[w] = lead[w] = 0xA5A5A5A5A5A5A5A5ull;
    run(hm, tx.t, n, docmask, n_words, start, lead);
    return 0;
}

// the first class table as the loader built it for this file: one flag byte per scalar value
extern "C" int blh_classes(const char* json, size_t json_len, uint8_t* flags_out /* [0x110000] */) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) flags_out[cp] = hm.uc_stage2[((size_t)hm.uc_stage1[cp >> 8] << 8) | (cp & 255u)];
    return 0;
}

// X of every scalar value as the CORE reads it: one char alone in a text, through bloom_word_classify (the byte table for ASCII, the class
// table for the rest)
extern "C" int blh_core_class(const char* json, size_t json_len, uint8_t* x_out /* [0x110000] */) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    if (hm.pretok != PT_BLOOM) return -1;
    uint32_t lut[256];
    for (uint32_t v = 0; v < 256; ++v) lut[v] = bloom_byte_flags(v);
    const uint64_t docmask[2] = {1, 0};
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) {
        x_out[cp] = 0;
        if (cp >= 0xD800u && cp < 0xE000u) continue;
        uint8_t enc[4];
        int64_t n;
        if (cp < 0x80u) { enc[0] = (uint8_t)cp; n = 1; }
        else if (cp < 0x800u) { enc[0] = (uint8_t)(0xC0u | (cp >> 6)); enc[1] = (uint8_t)(0x80u | (cp & 63u)); n = 2; }
        else if (cp < 0x10000u) { enc[0] = (uint8_t)(0xE0u | (cp >> 12)); enc[1] = (uint8_t)(0x80u | ((cp >> 6) & 63u)); enc[2] = (uint8_t)(0x80u | (cp & 63u)); n = 3; }
        else { enc[0] = (uint8_t)(0xF0u | (cp >> 18)); enc[1] = (uint8_t)(0x80u | ((cp >> 12) & 63u)); enc[2] = (uint8_t)(0x80u | ((cp >> 6) & 63u)); enc[3] = (uint8_t)(0x80u | (cp & 63u)); n = 4; }
        Text tx(enc, n);
        BloomWord m;
        bloom_word_classify(tx.t, n, docmask, lut, 0, hm.uc_stage1.data(), hm.uc_stage2.data(), m);
        const uint64_t all = (1ull << n) - 1ull;
        if ((m.X & all) == all) x_out[cp] = 1;
        else if (m.X & all) return -2;                       // (a char half in the class)
    }
    return 0;
}

#ifdef BLOOM_STANDALONE
static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    uint8_t tmp[1 << 16];
    size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) v.insert(v.end(), tmp, tmp + k);
    fclose(f);
    return v;
}

// bloom_check <tokenizer.json> <text bytes> <document offsets, int64 little endian> <expected start mask, uint64 little endian>:
// exit status 0 iff every word of the start mask is the expected one
int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s tokenizer.json text.bin offsets.bin starts.bin\n", argv[0]); return 2; }
    const std::vector<uint8_t> js = slurp(argv[1]), text = slurp(argv[2]), offb = slurp(argv[3]), expb = slurp(argv[4]);
    if (js.empty() || offb.size() < 8 || offb.size() % 8) { fprintf(stderr, "bad input files\n"); return 2; }
    std::vector<int64_t> off(offb.size() / 8);
    memcpy(off.data(), offb.data(), offb.size());
    const int64_t n = off.back(), n_docs = (int64_t)off.size() - 1;
    const size_t nw = (size_t)(n >> 6) + 1;
    if (n != (int64_t)text.size() || expb.size() != nw * 8) { fprintf(stderr, "the files do not fit each other\n"); return 2; }
    std::vector<uint64_t> st(nw), ld(nw), exp(nw);
    memcpy(exp.data(), expb.data(), expb.size());
    const int rc = blh_run((const char*)js.data(), js.size(), text.data(), n, off.data(), n_docs, st.data(), ld.data());
    if (rc) { fprintf(stderr, "blh_run: %d\n", rc); return 2; }
    size_t bad = 0;
    for (size_t w = 0; w < nw; ++w)
        if (st[w] != exp[w]) {
            if (!bad) fprintf(stderr, "word %zu: %016llx, expected %016llx\n", w, (unsigned long long)st[w], (unsigned long long)exp[w]);
            ++bad;
        }
    printf("%zu words, %zu differ\n", nw, bad);
    return bad ? 1 : 0;
}
#endif
