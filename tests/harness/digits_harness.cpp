// CPU harness for tokenizers_amd/csrc/pretok_digits_core.hpp: computes the start mask and the lead mask of a batch the way
// k_pretok_digits does -- one "lane" per 64-byte mask word, 256 lanes a workgroup, the packed `up` / `down` words handed between
// neighbouring lanes, digits_halo_classify at the workgroup's two ends -- with the tables of the tokenizer.json it is given (which must
// load as PT_DIGITS_GPT2).  Built as a shared library by tests/test_digits.py (g++, no GPU), and as a stand-alone program
// (-DDIGITS_STANDALONE, with -fsanitize=address,undefined) that reads the same inputs from files.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_model.hpp"
#include "pretok_digits_core.hpp"

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

template <bool INDIVIDUAL>
void run(const HostModel& hm, const uint8_t* t, int64_t n, const std::vector<uint64_t>& docmask, int64_t n_words, uint64_t* start, uint64_t* lead) {
    Gpt2Flags lut[256];
    for (uint32_t v = 0; v < 256; ++v) lut[v] = gpt2_byte_flags(v);
    const uint16_t* uc1 = hm.uc_stage1.data();
    const uint8_t* uc2 = hm.uc_stage2.data();
    const int64_t n_blocks = (n_words + WG - 1) / WG;
    std::vector<Gpt2Window> m((size_t)WG);
    std::vector<uint64_t> Nr((size_t)WG), up((size_t)WG);
    std::vector<DigitsSpill> sp((size_t)WG);
    std::vector<uint32_t> down((size_t)WG), down_nr((size_t)WG);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t w0 = b * WG;
        for (int64_t i = 0; i < WG; ++i) {
            sp[i] = digits_word_classify(t, n, docmask.data(), lut, w0 + i, uc1, uc2, m[i], &Nr[i]);
            up[i] = digits_pack_up<INDIVIDUAL>(m[i], Nr[i], sp[i]);
            down[i] = gpt2_pack_down(m[i]);
            down_nr[i] = (uint32_t)Nr[i] & 0xFFu;
        }
        // the two ends of the workgroup: threads 0 and 1 of the kernel
        uint64_t edge_up = 0;
        uint32_t edge_down = 0, edge_down_nr = 0;
        {
            DigitsSpill hs{{0, 0, 0}, 0};
            uint32_t nr8 = 0;
            if (w0 > 0 && (w0 << 6) < n) {
                const Gpt2Halo h = digits_halo_classify<INDIVIDUAL>(t, n, docmask.data(), lut, (w0 << 6) - 8, uc1, uc2, &hs, &nr8);
                edge_up = digits_pack_up(h, hs);
            }
            const int64_t pos = (w0 + WG) << 6;
            if (pos < n) {
                const Gpt2Halo h = digits_halo_classify<INDIVIDUAL>(t, n, docmask.data(), lut, pos, uc1, uc2, &hs, &nr8);
                edge_down = gpt2_pack_down(h.L, h.S, h.C, h.D);
                edge_down_nr = nr8;
            }
        }
        for (int64_t i = 0; i < WG; ++i) {
            const int64_t w = w0 + i;
            Gpt2Window mw = m[i];
            uint64_t nr = Nr[i];
            const Gpt2Halo hl = digits_take_left<INDIVIDUAL>(i == 0 ? edge_up : up[i - 1], w, mw, nr);
            const Gpt2Halo hr = digits_take_right<INDIVIDUAL>(i == WG - 1 ? edge_down : down[i + 1], i == WG - 1 ? edge_down_nr : down_nr[i + 1], w, n, sp[i]);
            uint64_t ld = 0;
            const uint64_t out = gpt2_word_starts(mw, hl, hr, t, w, &ld);
            if (w < n_words) { start[w] = out; lead[w] = ld; }
        }
    }
}
}  // namespace

// start / lead: (n >> 6) + 1 words each.  -1: the file does not load as PT_DIGITS_GPT2
extern "C" int dgh_run(const char* json, size_t json_len, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs, uint64_t* start, uint64_t* lead) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    if (hm.pretok != PT_DIGITS_GPT2) return -1;
    const int64_t n_words = (n >> 6) + 1;
    std::vector<uint64_t> docmask((size_t)n_words + 1, 0);
    for (int64_t d = 0; d < n_docs; ++d)
        if (doc_off[d] < n) docmask[doc_off[d] >> 6] |= 1ull << (doc_off[d] & 63);
    Text tx(text, n);
    for (int64_t w = 0; w < n_words; ++w) start[w] = lead[w] = 0xA5A5A5A5A5A5A5A5ull;
    if (hm.digits_individual) run<true>(hm, tx.t, n, docmask, n_words, start, lead);
    else run<false>(hm, tx.t, n, docmask, n_words, start, lead);
    return 0;
}

// the first class table as the loader built it for this file: one flag byte per scalar value
extern "C" int dgh_classes(const char* json, size_t json_len, uint8_t* flags_out /* [0x110000] */) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) flags_out[cp] = hm.uc_stage2[((size_t)hm.uc_stage1[cp >> 8] << 8) | (cp & 255u)];
    return 0;
}

#ifdef DIGITS_STANDALONE
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

// digits_check <tokenizer.json> <text bytes> <document offsets, int64 little endian> <expected start mask, uint64 little endian>:
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
    const int rc = dgh_run((const char*)js.data(), js.size(), text.data(), n, off.data(), n_docs, st.data(), ld.data());
    if (rc) { fprintf(stderr, "dgh_run: %d\n", rc); return 2; }
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
