// CPU harness for the token compaction: tokenizers_amd/csrc/kernels/{results,scan_util,output}.hip compiled for the host, UNCHANGED, under
// the SIMT shim of tests/harness/simt/, and k_compact<CP_ITEMS_PER_LANE> launched directly on synthetic inputs at any grid and patience --
// the workgroups run one after the other here, so every total a workgroup needs from a LATER workgroup is one it has to compute itself.
// Built and used by tests/test_compact_prefix_core.py (as a shared library); with its own main() it is also a stand-alone program, which
// is how it is run under -fsanitize=address,undefined: every buffer is a heap block of exactly the size the host code reserves.
// Test infrastructure; nothing in the product includes this.
#include <hip/hip_runtime.h>   // the shim (-I tests/harness/simt)

#include <cstdint>
#include <cstdio>
#include <vector>

#include "device_utils.hpp"
#include "kernels.hpp"
#include "overflow_core.hpp"
#include "tables.hpp"

namespace tkamd {
struct __attribute__((packed, aligned(1))) Unaligned4 { uint32_t v; };
struct __attribute__((packed, aligned(1))) Unaligned16 { uint32_t a, b, c, d; };
// (the helpers kernels.hip itself defines in front of its slices: the host forms)
inline uint32_t uc_flags(uint32_t cp, const uint16_t* uc1, const uint8_t* uc2) { return cp >= 0x110000u ? 0u : uc2[((uint32_t)uc1[cp >> 8] << 8) | (cp & 255u)]; }
inline uint32_t utf8_global(const uint8_t* text, int64_t i, uint32_t* len) {
    const uint32_t w = ((const Unaligned4*)(text + i))->v;
    const uint32_t b0 = w & 0xFFu, b1 = (w >> 8) & 0x3Fu, b2 = (w >> 16) & 0x3Fu, b3 = (w >> 24) & 0x3Fu;
    if (b0 < 0x80u) { *len = 1; return b0; }
    if (b0 < 0xE0u) { *len = 2; return ((b0 & 0x1Fu) << 6) | b1; }
    if (b0 < 0xF0u) { *len = 3; return ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2; }
    *len = 4;
    return ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3;
}
template <class T> inline T load_nt(const T* p) { return *p; }
template <class T> inline void store_nt(T* p, T v) { *p = v; }
#include "kernels/results.hip"
#include "kernels/scan_util.hip"
#include "kernels/output.hip"
}  // namespace tkamd

using namespace tkamd;

namespace {
struct Result {
    std::vector<uint32_t> ids, pt_tokoff;
    std::vector<int64_t> tok_offsets;
    std::vector<unsigned long long> state;
    int64_t n_tok = -1, n_chunks = 0;
} R;
}  // namespace

extern "C" {

// tok0[P], rows[n_rows] (16 bytes each; row 0 exists), tmp_ids[n_tmp], doc_pt[n_docs + 1] (the last entry is P); T: the token count the
// caller expects (ids gets exactly that many words).  grid / patience: as launch_compact takes them from its hooks.
int cp_run(const uint32_t* tok0, int64_t P, const uint32_t* rows, int64_t n_rows, const uint32_t* tmp_ids, int64_t n_tmp, const uint32_t* doc_pt, int64_t n_docs,
           int64_t T, int grid, uint32_t patience, int want_pt_tokoff) {
    R = Result{};
    const int64_t n_chunks = (P + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
    R.n_chunks = n_chunks;
    // the sizes capi/pipeline.cpp reserves for a text of P bytes (the least that can hold P pre-tokens)
    std::vector<uint32_t> v_tok0((size_t)P + 4, 0u), v_tmp((size_t)n_tmp + 4, 0u), v_chunk_lo((size_t)P / COMPACT_CHUNK + 4, 0u), v_doc_pt(doc_pt, doc_pt + n_docs + 1);
    std::vector<uint4> v_rows((size_t)n_rows);
    for (int64_t i = 0; i < P; ++i) v_tok0[(size_t)i] = tok0[i];
    for (int64_t i = 0; i < n_tmp; ++i) v_tmp[(size_t)i] = tmp_ids[i];
    for (int64_t i = 0; i < n_rows; ++i) v_rows[(size_t)i] = make_uint4(rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]);
    for (int64_t c = 0, d = 0; c <= n_chunks; ++c) {                  // kernels/scan_emit.hip k_doc_first_pretok: the first document that starts at or behind the chunk
        while (d <= n_docs && (int64_t)doc_pt[d] < c * COMPACT_CHUNK) ++d;
        v_chunk_lo[(size_t)c] = (uint32_t)d;
    }
    R.state.assign(lb_state_words((size_t)P / COMPACT_CHUNK + 4), 0ull);
    R.ids.assign((size_t)T, 0xDEADBEEFu);
    R.tok_offsets.assign((size_t)n_docs + 1, -1);
    if (want_pt_tokoff) R.pt_tokoff.assign((size_t)P, 0xDEADBEEFu);
    const int64_t n_pretok = P;
    hipLaunchKernelGGL(k_compact<CP_ITEMS_PER_LANE>, dim3(grid), dim3(CP_NT), 0, nullptr, v_tok0.data(), v_rows.data(), v_rows.data(), v_tmp.data(), &n_pretok, R.state.data(),
                       &R.n_tok, want_pt_tokoff ? R.pt_tokoff.data() : nullptr, R.ids.data(), v_chunk_lo.data(), v_doc_pt.data(), n_docs, R.tok_offsets.data(),
                       (unsigned long long*)nullptr, patience, (uint8_t*)nullptr);
    return 0;
}
int64_t cp_n_tok(void) { return R.n_tok; }
const uint32_t* cp_ids(void) { return R.ids.data(); }
const uint32_t* cp_pt_tokoff(void) { return R.pt_tokoff.data(); }
const int64_t* cp_tok_offsets(void) { return R.tok_offsets.data(); }
// the state after the run: chunk c's word, group g's word (count << 56 | sum)
unsigned long long cp_state_word(int64_t c) { return R.state[(size_t)c]; }
unsigned long long cp_group_word(int64_t g) { return R.state[lb_group_base((size_t)R.n_chunks) + (size_t)g * LB_GROUP_STRIDE]; }
uint32_t cp_default_patience(void) { return LB_PATIENCE; }
int cp_chunk(void) { return COMPACT_CHUNK; }
int cp_stage(void) { return CpShape<CP_ITEMS_PER_LANE>::STAGE; }

}  // extern "C"

// ---- the stand-alone program: a batch of its own making against a plain sequential loop, over a handful of chunk counts, grids and
// patiences (what the sanitizer build runs) ----
namespace {
struct Gen {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};
int run_case(int64_t n_chunks, int64_t last, int grid, uint32_t patience) {
    const int64_t P = (n_chunks - 1) * COMPACT_CHUNK + last;
    Gen g{(uint64_t)(n_chunks * 1000003 + grid * 101 + last)};
    std::vector<uint32_t> tok0((size_t)P), rows(4, 0u), tmp(1, 0u), exp_ids, cnt((size_t)P);
    const int64_t fat = n_chunks / 2;                                  // the chunk whose tokens do not fit the LDS stage
    for (int64_t p = 0; p < P; ++p) {
        const uint32_t r = g.next() % 100u, id = g.next() & 0xFFFFFu;
        uint32_t c = r < 70u ? 1u : r < 75u ? 0u : r < 95u ? 1u + g.next() % 4u : r < 98u ? 7u : 40u;
        if (p / COMPACT_CHUNK == fat && p % 8 == 0) c = 40u;
        cnt[(size_t)p] = c;
        if (r < 70u && c == 1u) { tok0[(size_t)p] = TOK_ONE | id; exp_ids.push_back(id); continue; }
        tok0[(size_t)p] = TOK_ROW | (uint32_t)(rows.size() / 4);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (c <= 4u) {
            for (uint32_t j = 0; j < c; ++j) { w[j] = (id + j) & 0xFFFFFu; exp_ids.push_back(w[j]); }
            w[0] |= c << ROW_CNT_SHIFT;
        } else {
            const uint32_t s = (uint32_t)tmp.size() - 1u;              // ids 1.. in tmp_ids[s + 1 ..]
            w[0] = id | (ROW_CNT_MORE << ROW_CNT_SHIFT); w[1] = s; w[2] = c;
            exp_ids.push_back(id);
            for (uint32_t j = 1; j < c; ++j) { tmp.push_back((id + j) & 0xFFFFFu); exp_ids.push_back((id + j) & 0xFFFFFu); }
            tmp.push_back(0u);
        }
        rows.insert(rows.end(), w, w + 4);
    }
    std::vector<uint32_t> doc_pt;
    for (int64_t p = 0; p < P; p += 1 + g.next() % 700u) doc_pt.push_back((uint32_t)p);
    for (int64_t c = 0; c * COMPACT_CHUNK <= P; c += 3) { doc_pt.push_back((uint32_t)(c * COMPACT_CHUNK)); doc_pt.push_back((uint32_t)(c * COMPACT_CHUNK)); }      // empty documents at chunk edges
    doc_pt.push_back((uint32_t)P); doc_pt.push_back((uint32_t)P);      // ... and behind the last pre-token
    std::sort(doc_pt.begin(), doc_pt.end());
    const int64_t n_docs = (int64_t)doc_pt.size() - 1;
    std::vector<int64_t> pre((size_t)P + 1, 0);
    for (int64_t p = 0; p < P; ++p) pre[(size_t)p + 1] = pre[(size_t)p] + cnt[(size_t)p];
    cp_run(tok0.data(), P, rows.data(), (int64_t)rows.size() / 4, tmp.data(), (int64_t)tmp.size(), doc_pt.data(), n_docs, pre[(size_t)P], grid, patience, 1);
    int bad = 0;
    bad += R.n_tok != pre[(size_t)P];
    bad += R.ids != exp_ids;
    for (int64_t d = 0; d <= n_docs; ++d) bad += R.tok_offsets[(size_t)d] != pre[doc_pt[(size_t)d]];
    for (int64_t p = 0; p < P; ++p) bad += R.pt_tokoff[(size_t)p] != (uint32_t)pre[(size_t)p];
    for (int64_t gr = 0; gr < n_chunks / LB_GROUP_CHUNKS; ++gr) bad += (cp_group_word(gr) >> 56) != 64ull;
    printf("chunks %lld last %lld grid %d patience %u: %s\n", (long long)n_chunks, (long long)last, grid, patience, bad ? "MISMATCH" : "ok");
    return bad != 0;
}
}  // namespace

int main() {
    int bad = 0;
    const int64_t chunks[] = {1, 2, 64, 65, 129};
    const int grids[] = {1, 3, 64, 65, 1000};
    for (int64_t n : chunks)
        for (int gr : grids) {
            bad += run_case(n, COMPACT_CHUNK, gr, 8u);
            bad += run_case(n, 1, gr, 0u);
        }
    bad += run_case(129, 77, 2, LB_PATIENCE);
    bad += run_case(4200, 5, 4300, 8u);                                // a range of more than 64 whole groups: a second round of group words
    printf(bad ? "FAILED\n" : "ALL_OK\n");
    return bad != 0;
}
