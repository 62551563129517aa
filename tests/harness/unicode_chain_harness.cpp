// CPU harness for the NFD / Lowercase / StripAccents normalizer chains (NORM_CHAIN): loads a tokenizer.json with the loader the library
// runs and normalizes a batch of strings (each one piece) by HostModel::chain_normalize -- the per-char tables k_bn_count / k_bn_write read
// for a chain that is context free per char, the segment core of nfc_core.hpp in its NFD mode where NFD stays visible.  Built as a shared
// library with g++ by tests/test_unicode_chain.py, which holds it against the reference wheel.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"

using namespace tkamd;

namespace {
HostModel g_model;
std::string g_error;
}  // namespace

extern "C" {

// 0: loaded; -1: refused (uch_error says why)
int uch_load(const char* json, int64_t len) {
    try {
        g_model = HostModel::from_json(json, (size_t)len);
        if (g_model.norm != NORM_CHAIN) { g_error = "the file has no NFD / Lowercase / StripAccents normalizer"; return -1; }
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return -1;
    }
}
const char* uch_error() { return g_error.c_str(); }
// NFD_MODE | where Lowercase stands (nfc_core.hpp), 0 for a chain that is context free per char
uint32_t uch_nfd_mode() { return g_model.nfd_mode(); }

// documents [off[d], off[d + 1]) of text; out / out_off: the normalized documents as a CSR (out holds out_cap bytes); norig: per output
// byte the first byte of the source char it is aligned to, relative to its document; status[d]: 1 = refused (a segment beyond 48).
// Returns the bytes written, or -1 if out_cap is too small.
int64_t uch_normalize_batch(const uint8_t* text, const int64_t* off, int64_t count, uint8_t* out, int64_t out_cap, int64_t* out_off, uint32_t* norig,
                            uint8_t* status) {
    int64_t w = 0;
    std::vector<uint32_t> al;
    for (int64_t d = 0; d < count; ++d) {
        const std::string s((const char*)text + off[d], (size_t)(off[d + 1] - off[d]));
        bool refused = false;
        al.clear();
        const std::string o = g_model.chain_normalize(s, &al, &refused);
        out_off[d] = w;
        if (w + (int64_t)o.size() > out_cap) return -1;
        if (!o.empty()) memcpy(out + w, o.data(), o.size());
        if (norig && !al.empty()) memcpy(norig + w, al.data(), al.size() * 4);
        w += (int64_t)o.size();
        status[d] = refused ? 1 : 0;
    }
    out_off[count] = w;
    return w;
}

}  // extern "C"
