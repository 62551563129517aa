// CPU harness for tokenizers_amd/csrc/pretok_ds3_core.hpp: runs ds3_window_starts -- the exact function every lane of k_pretok_ds3_lane
// executes -- over a whole batch, one 64-byte window per 48 bytes of text, the way the kernel tiles it, and ds3_doc_starts -- the whole of
// k_pretok_ds3_slow -- document by document.  Built and driven by tests/test_split_chain.py (g++, no GPU).
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_model.hpp"
#include "pretok_ds3_core.hpp"

using namespace tkamd;

namespace {
bool load(const char* json, size_t json_len, HostModel* hm) {
    try {
        *hm = HostModel::from_json(json, json_len);
    } catch (const std::exception&) {
        return false;
    }
    return hm->pretok == PT_SPLIT_CHAIN && !hm->ucc_stage1.empty();
}
}  // namespace

// window core: start_out / unres_out one byte per text byte
extern "C" int ds3h_run(const char* json, size_t json_len, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs,
                        uint8_t* start_out, uint8_t* unres_out) {
    HostModel hm;
    if (!load(json, json_len, &hm)) return -1;
    std::vector<uint8_t> docstart((size_t)n + 64, 0);
    for (int64_t d = 0; d < n_docs; ++d)
        if (doc_off[d] < n) docstart[doc_off[d]] = 1;
    // padded copy: the kernel's text carries 64 readable bytes after its end and the first window starts 8 bytes early
    std::vector<uint8_t> buf((size_t)n + 64 + 128, 0);
    uint8_t* t = buf.data() + 64;
    memcpy(t, text, (size_t)n);
    L3Flags lut[256];
    for (uint32_t v = 0; v < 256; ++v) lut[v] = ds3_byte_flags(v);
    for (int64_t a = 0; a < n; a += L3W_MAIN) {
        const int64_t base = a - L3W_HALO;
        L3Window w{};
        for (int i = 0; i < 64; ++i) {
            const int64_t g = base + i;
            if (g < 0 || g >= n) continue;
            const L3Flags f = lut[t[g]];
            const uint64_t bit = 1ull << i;
            w.V |= bit;
            if (f.x & 1u) w.L |= bit;
            if (f.x & (1u << 8)) w.N |= bit;
            if (f.x & (1u << 16)) w.W |= bit;
            if (f.x & (1u << 24)) w.R |= bit;
            if (f.y & 1u) w.SP |= bit;
            if (f.y & (1u << 8)) w.C |= bit;
            if (f.y & (1u << 16)) w.AP |= bit;
            if (f.y & (1u << 24)) w.MU |= bit;
            if (docstart[g]) w.D |= bit;
        }
        uint64_t st = 0, un = 0;
        ds3_window_starts(w, t, base, hm.uc_stage1.data(), hm.uc_stage2.data(), hm.ucc_stage1.data(), hm.ucc_stage2.data(), &st, &un);
        for (int i = L3W_HALO; i < L3W_HALO + L3W_MAIN; ++i) {
            const int64_t g = base + i;
            if (g < n) { start_out[g] = (st >> i) & 1; unres_out[g] = (un >> i) & 1; }
        }
    }
    return 0;
}

// the sequential matcher alone: start_out one byte per text byte
extern "C" int ds3h_seq(const char* json, size_t json_len, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs, uint8_t* start_out) {
    HostModel hm;
    if (!load(json, json_len, &hm)) return -1;
    const Ds3Seq q{hm.uc_stage1.data(), hm.uc_stage2.data(), hm.ucc_stage1.data(), hm.ucc_stage2.data()};
    memset(start_out, 0, (size_t)n);
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t a = doc_off[d], b = doc_off[d + 1];
        ds3_doc_starts(q, text + a, b - a, [&](int64_t p) { start_out[a + p] = 1; });
    }
    return 0;
}

// the second class table as the loader built it: one flag byte per scalar value
extern "C" int ds3h_classes(const char* json, size_t json_len, uint8_t* flags_out /* [0x110000] */) {
    HostModel hm;
    if (!load(json, json_len, &hm)) return -1;
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) flags_out[cp] = (uint8_t)l3_uc_flags(cp, hm.ucc_stage1.data(), hm.ucc_stage2.data());
    return 0;
}
