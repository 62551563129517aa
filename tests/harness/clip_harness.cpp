// CPU harness for the CLIP layout's two cores.
//   clh_run: tokenizers_amd/csrc/pretok_clip_core.hpp -- the start, end and lead masks of a batch the way k_pretok_clip computes them: one
//   "lane" per 64-byte mask word, 256 lanes a workgroup, the packed `up` / `down` words handed between neighbouring lanes,
//   gpt2_halo_classify at the workgroup's two ends -- with the tables of the tokenizer.json it is given (which must load as PT_CLIP).
//   clh_normalize: the NFC_LOWER mode of tokenizers_amd/csrc/nfc_core.hpp over one piece, through HostModel::nfc_normalize -- the text
//   and, per output byte, the first byte of the source char it is aligned to.
// Built as a shared library by tests/test_clip.py (g++, no GPU), and as a stand-alone program (-DCLIP_STANDALONE, for a sanitizer build)
// that reads the same inputs from files.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"
#include "pretok_clip_core.hpp"

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

void run(const HostModel& hm, const uint8_t* t, int64_t n, const std::vector<uint64_t>& docmask, int64_t n_words, uint64_t* start, uint64_t* end, uint64_t* lead) {
    Gpt2Flags lut[256];
    for (uint32_t v = 0; v < 256; ++v) lut[v] = gpt2_byte_flags(v);
    const uint16_t* uc1 = hm.uc_stage1.data();
    const uint8_t* uc2 = hm.uc_stage2.data();
    const int64_t n_blocks = (n_words + WG - 1) / WG;
    std::vector<Gpt2Window> m((size_t)WG);
    std::vector<Gpt2Spill> sp((size_t)WG);
    std::vector<uint64_t> up((size_t)WG);
    std::vector<uint32_t> down((size_t)WG);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t w0 = b * WG;
        for (int64_t i = 0; i < WG; ++i) {
            sp[i] = gpt2_word_classify(t, n, docmask.data(), lut, w0 + i, uc1, uc2, m[i]);
            up[i] = gpt2_pack_up(m[i], sp[i]);
            down[i] = gpt2_pack_down(m[i]);
        }
        // the two ends of the workgroup: threads 0 and 1 of the kernel
        uint64_t edge_up = 0;
        uint32_t edge_down = 0;
        {
            Gpt2Spill hs{0, 0, 0};
            if (w0 > 0 && (w0 << 6) <= n) {
                const Gpt2Halo h = gpt2_halo_classify(t, n, docmask.data(), lut, (w0 << 6) - 8, uc1, uc2, &hs);
                edge_up = gpt2_pack_up(h.L, h.N, h.S, h.SP, h.AP, h.D, hs);
            }
            const int64_t pos = (w0 + WG) << 6;
            if (pos < n) {
                const Gpt2Halo h = gpt2_halo_classify(t, n, docmask.data(), lut, pos, uc1, uc2, &hs);
                edge_down = gpt2_pack_down(h.L, h.S, h.C, h.D);
            }
        }
        for (int64_t i = 0; i < WG; ++i) {
            const int64_t w = w0 + i;
            Gpt2Window mw = m[i];
            const Gpt2Halo hl = gpt2_take_left(i == 0 ? edge_up : up[i - 1], w, mw);
            const Gpt2Halo hr = gpt2_take_right(i == WG - 1 ? edge_down : down[i + 1], w, n, sp[i]);
            uint64_t st = 0, en = 0, ld = 0;
            clip_word_masks(mw, hl, hr, t, w, n, &st, &en, &ld);
            if (w < n_words) { start[w] = st; end[w] = en; lead[w] = ld; }
        }
    }
}
}  // namespace

// start / end / lead: (n >> 6) + 1 words each.  -1: the file does not load as PT_CLIP
extern "C" int clh_run(const char* json, size_t json_len, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs, uint64_t* start, uint64_t* end, uint64_t* lead) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    if (hm.pretok != PT_CLIP) return -1;
    const int64_t n_words = (n >> 6) + 1;
    std::vector<uint64_t> docmask((size_t)n_words + 1, 0);
    for (int64_t d = 0; d < n_docs; ++d)
        if (doc_off[d] < n) docmask[doc_off[d] >> 6] |= 1ull << (doc_off[d] & 63);
    Text tx(text, n);
    for (int64_t w = 0; w < n_words; ++w) start[w] = end[w] = lead[w] = 0xA5A5A5A5A5A5A5A5ull;
    run(hm, tx.t, n, docmask, n_words, start, end, lead);
    return 0;
}

// the normalizer of the file over one piece: out (cap bytes) and norig (cap words).  Returns the output's length, -1: the file does not
// load with the NFC + Lowercase chain, -2: refused (more than 48 chars in a segment), -3: cap too small
extern "C" int64_t clh_normalize(const char* json, size_t json_len, const uint8_t* text, int64_t n, uint8_t* out, uint32_t* norig, int64_t cap) {
    static HostModel hm;
    static std::string loaded;
    try {
        if (loaded != std::string(json, json_len)) {
            hm = HostModel::from_json(json, json_len);
            loaded.assign(json, json_len);
        }
    } catch (const std::exception&) {
        return -1;
    }
    if (!hm.nfc_lower) return -1;
    bool refused = false;
    std::vector<uint32_t> no;
    std::string padded((const char*)text, (size_t)n);
    const std::string o = hm.nfc_normalize(padded, &no, &refused);
    if (refused) return -2;
    if ((int64_t)o.size() > cap) return -3;
    memcpy(out, o.data(), o.size());
    memcpy(norig, no.data(), no.size() * 4);
    return (int64_t)o.size();
}

#ifdef CLIP_STANDALONE
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

// clip_check <tokenizer.json> <text bytes> <document offsets, int64 little endian> <expected start mask, then end mask, uint64 little endian>:
// exit status 0 iff every word of both masks is the expected one
int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s tokenizer.json text.bin offsets.bin masks.bin\n", argv[0]); return 2; }
    const std::vector<uint8_t> js = slurp(argv[1]), text = slurp(argv[2]), offb = slurp(argv[3]), expb = slurp(argv[4]);
    if (js.empty() || offb.size() < 8 || offb.size() % 8) { fprintf(stderr, "bad input files\n"); return 2; }
    std::vector<int64_t> off(offb.size() / 8);
    memcpy(off.data(), offb.data(), offb.size());
    const int64_t n = off.back(), n_docs = (int64_t)off.size() - 1;
    const size_t nw = (size_t)(n >> 6) + 1;
    if (n != (int64_t)text.size() || expb.size() != 2 * nw * 8) { fprintf(stderr, "the files do not fit each other\n"); return 2; }
    std::vector<uint64_t> st(nw), en(nw), ld(nw), exp(2 * nw);
    memcpy(exp.data(), expb.data(), expb.size());
    const int rc = clh_run((const char*)js.data(), js.size(), text.data(), n, off.data(), n_docs, st.data(), en.data(), ld.data());
    if (rc) { fprintf(stderr, "clh_run: %d\n", rc); return 2; }
    size_t bad = 0;
    for (size_t w = 0; w < nw; ++w)
        if (st[w] != exp[w] || en[w] != exp[nw + w]) {
            if (!bad) fprintf(stderr, "word %zu: %016llx / %016llx, expected %016llx / %016llx\n", w, (unsigned long long)st[w], (unsigned long long)en[w],
                              (unsigned long long)exp[w], (unsigned long long)exp[nw + w]);
            ++bad;
        }
    printf("%zu words, %zu differ\n", nw, bad);
    return bad ? 1 : 0;
}
#endif
