// CPU harness for the word-aligned form of tokenizers_amd/csrc/pretok_gpt2_core.hpp (gpt2_word_classify, gpt2_halo_classify,
// gpt2_take_left / gpt2_take_right, gpt2_word_starts): computes the start mask and the lead mask of a text twice,
//   new: one "lane" per mask word, the halos passed the way k_pretok_gpt2_seq passes them -- packed `up` / `down` words between the
//        lanes of a 256-lane workgroup, gpt2_halo_classify at the workgroup's two ends;
//   old: gpt2_lane_starts, four lanes' 48 bits assembled into three words exactly as l3_harness.cpp's g2h_run does,
// and hands both back.  Built as a shared library by tests/test_pretok_gpt2_words.py, and as a stand-alone program
// (-DG2W_STANDALONE, with -fsanitize=address,undefined) that reads the same inputs from files.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"
#include "pretok_gpt2_core.hpp"

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

void run_new(const HostModel& hm, const uint8_t* t, int64_t n, const std::vector<uint64_t>& docmask, int64_t n_words, uint64_t* start, uint64_t* lead) {
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
            if (w0 > 0 && (w0 << 6) < n) {
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
            uint64_t ld = 0;
            const uint64_t out = gpt2_word_starts(mw, hl, hr, t, w, &ld);
            if (w < n_words) { start[w] = out; lead[w] = ld; }
        }
    }
}

void run_old(const HostModel& hm, const uint8_t* t, int64_t n, const std::vector<uint64_t>& docmask, int64_t n_words, uint64_t* start, uint64_t* lead) {
    Gpt2Flags lut[256];
    for (uint32_t v = 0; v < 256; ++v) lut[v] = gpt2_byte_flags(v);
    const int64_t n_lanes = ((n + 1 + 256 * G2W_MAIN - 1) / (256 * G2W_MAIN)) * 256;
    std::vector<uint64_t> out((size_t)n_lanes + 1, 0), ld((size_t)n_lanes + 1, 0);
    for (int64_t lane = 0; lane < n_lanes; ++lane)
        out[lane] = gpt2_lane_starts(t, n, n_words, docmask.data(), lut, lane, hm.uc_stage1.data(), hm.uc_stage2.data(), &ld[lane]);
    for (int64_t lane = 0; lane < n_lanes; ++lane) {
        const int q = (int)(lane & 3);
        if (q == 3) continue;
        const int64_t word = 3 * (lane >> 2) + q;
        const bool last = (lane & 63) == 63;
        if (word < n_words) {
            start[word] = (out[lane] >> (16 * q)) | ((last ? 0 : out[lane + 1]) << (G2W_MAIN - 16 * q));
            lead[word] = (ld[lane] >> (16 * q)) | ((last ? 0 : ld[lane + 1]) << (G2W_MAIN - 16 * q));
        }
    }
}
}  // namespace

// start_new / lead_new / start_old / lead_old: (n >> 6) + 1 words each
extern "C" int g2w_run(const char* json, size_t json_len, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs,
                       uint64_t* start_new, uint64_t* lead_new, uint64_t* start_old, uint64_t* lead_old) {
    HostModel hm;
    try {
        hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return -1;
    }
    const int64_t n_words = (n >> 6) + 1;
    std::vector<uint64_t> docmask((size_t)n_words + 1, 0);
    for (int64_t d = 0; d < n_docs; ++d)
        if (doc_off[d] < n) docmask[doc_off[d] >> 6] |= 1ull << (doc_off[d] & 63);
    Text tx(text, n);
    for (int64_t w = 0; w < n_words; ++w) start_new[w] = lead_new[w] = start_old[w] = lead_old[w] = 0xA5A5A5A5A5A5A5A5ull;
    run_new(hm, tx.t, n, docmask, n_words, start_new, lead_new);
    run_old(hm, tx.t, n, docmask, n_words, start_old, lead_old);
    return 0;
}

#ifdef G2W_STANDALONE
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

// g2w_check <tokenizer.json> <text bytes> <document offsets, int64 little endian>: exit status 0 iff both forms agree on every word
int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s tokenizer.json text.bin offsets.bin\n", argv[0]); return 2; }
    const std::vector<uint8_t> js = slurp(argv[1]), text = slurp(argv[2]), offb = slurp(argv[3]);
    if (js.empty() || offb.size() < 8 || offb.size() % 8) { fprintf(stderr, "bad input files\n"); return 2; }
    std::vector<int64_t> off(offb.size() / 8);
    memcpy(off.data(), offb.data(), offb.size());
    const int64_t n = off.back(), n_docs = (int64_t)off.size() - 1;
    if (n != (int64_t)text.size()) { fprintf(stderr, "offsets end at %lld, the text has %zu bytes\n", (long long)n, text.size()); return 2; }
    const size_t nw = (size_t)(n >> 6) + 1;
    std::vector<uint64_t> sn(nw), ln(nw), so(nw), lo(nw);
    const int rc = g2w_run((const char*)js.data(), js.size(), text.data(), n, off.data(), n_docs, sn.data(), ln.data(), so.data(), lo.data());
    if (rc) { fprintf(stderr, "g2w_run: %d\n", rc); return 2; }
    size_t bad = 0;
    for (size_t w = 0; w < nw; ++w)
        if (sn[w] != so[w] || ln[w] != lo[w]) {
            if (!bad) fprintf(stderr, "word %zu: start %016llx / %016llx, lead %016llx / %016llx (new / old)\n", w, (unsigned long long)sn[w],
                              (unsigned long long)so[w], (unsigned long long)ln[w], (unsigned long long)lo[w]);
            ++bad;
        }
    printf("%zu words, %zu differ\n", nw, bad);
    return bad ? 1 : 0;
}
#endif
