// CPU harness for tokenizers_amd/csrc/precompiled_core.hpp: loads a precompiled_charsmap the way the loader does
// (HostModel::set_precompiled: every refusal of a malformed blob) and normalizes a batch of strings (each one piece) with the core the
// kernels run -- HostModel::precompiled_normalize.  Built as a shared library by tests/test_precompiled.py, which holds both against the
// reference wheel; built with -DPCH_MAIN as a stand-alone program, it runs a file of blobs and documents through the same two calls (the
// sanitizer run of the same test: every document in an allocation of exactly its size).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"
#include "precompiled_core.hpp"

using namespace tkamd;

namespace {
HostModel g_model;
std::string g_error;
}  // namespace

extern "C" {

// 0: loaded; -1: refused (pch_error says why)
int pch_load(const uint8_t* blob, int64_t len) {
    try {
        g_model = HostModel();
        g_model.set_precompiled(std::string((const char*)blob, (size_t)len));
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return -1;
    }
}
const char* pch_error() { return g_error.c_str(); }
// the most output bytes a source byte can stand for, as the loader found it: what the host bounds the normalized text by
uint32_t pch_growth() { return g_model.pc_growth; }

// documents [off[d], off[d + 1]) of text; out / out_off: the normalized documents as a CSR (out holds out_cap bytes); norig: per output
// byte the first byte of the source char it is aligned to, relative to its document.  Returns the bytes written, or -1 if out_cap is too small.
int64_t pch_normalize_batch(const uint8_t* text, const int64_t* off, int64_t count, uint8_t* out, int64_t out_cap, int64_t* out_off, uint32_t* norig) {
    int64_t w = 0;
    std::vector<uint32_t> al;
    for (int64_t d = 0; d < count; ++d) {
        const std::string s((const char*)text + off[d], (size_t)(off[d + 1] - off[d]));
        const std::string o = g_model.precompiled_normalize(s, &al);
        out_off[d] = w;
        if (w + (int64_t)o.size() > out_cap) return -1;
        memcpy(out + w, o.data(), o.size());
        if (norig && !al.empty()) memcpy(norig + w, al.data(), al.size() * 4);
        w += (int64_t)o.size();
    }
    out_off[count] = w;
    return w;
}

}  // extern "C"

#ifdef PCH_MAIN
// file: u32 n_blobs, {u32 len, bytes}, u32 n_docs, {u32 len, bytes} -- every document through every blob that loads
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    auto rd = [&](std::vector<std::vector<uint8_t>>& v) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) return false;
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t l = 0;
            if (fread(&l, 4, 1, f) != 1) return false;
            std::vector<uint8_t> b(l);
            if (l && fread(b.data(), 1, l, f) != l) return false;
            v.push_back(std::move(b));
        }
        return true;
    };
    std::vector<std::vector<uint8_t>> blobs, docs;
    if (!rd(blobs) || !rd(docs)) return 2;
    fclose(f);
    size_t loaded = 0, bytes = 0;
    for (const auto& b : blobs) {
        if (pch_load(b.data(), (int64_t)b.size()) != 0) continue;
        ++loaded;
        for (const auto& d : docs) {
            std::vector<uint32_t> al;
            bytes += g_model.precompiled_normalize(std::string((const char*)d.data(), d.size()), &al).size();
        }
    }
    printf("blobs %zu loaded %zu docs %zu output bytes %zu\n", blobs.size(), loaded, docs.size(), bytes);
    return 0;
}
#endif
