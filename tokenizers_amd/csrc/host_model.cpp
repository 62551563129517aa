// tokenizer.json -> flat tables.  See host_model.hpp.
#include "host_model.hpp"
#include "bert_norm_core.hpp"
#include "nfc_core.hpp"
#include "precompiled_core.hpp"
#include "pretok_bloom_core.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <set>
#include <unordered_map>

#include "json.hpp"

namespace tkamd {

// Two-choice (cuckoo) placement of keys with hashes h1 into a table of mask + 1 slots (word_slot_a / word_slot_b, tables.hpp): a key
// goes to its slot a, else b, else it evicts the tenant of a, who moves to ITS other slot, and so on; a walk that does not end within
// the bound means an unlucky seed (at load factor <= 0.4 that is rare).  tenant[slot] = index of the key, or 0xFFFFFFFF.
bool cuckoo_place(const std::vector<uint32_t>& h1, uint32_t mask, std::vector<uint32_t>* tenant) {
    tenant->assign((size_t)mask + 1, 0xFFFFFFFFu);
    std::vector<uint32_t>& tn = *tenant;
    for (size_t i = 0; i < h1.size(); ++i) {
        uint32_t cur = (uint32_t)i, pos = word_slot_a(h1[cur], mask);
        if (tn[pos] != 0xFFFFFFFFu && tn[word_slot_b(h1[cur], mask)] == 0xFFFFFFFFu) pos = word_slot_b(h1[cur], mask);
        for (int kicks = 0;; ++kicks) {
            if (tn[pos] == 0xFFFFFFFFu) { tn[pos] = cur; break; }
            if (kicks == 512) return false;
            std::swap(cur, tn[pos]);                              // cur takes the slot; its tenant moves to ITS other slot
            pos = pos == word_slot_a(h1[cur], mask) ? word_slot_b(h1[cur], mask) : word_slot_a(h1[cur], mask);
        }
    }
    return true;
}

// Hash-and-displace (CHD) perfect hash: keys are bucketed by h1, buckets are placed largest first, each one
// searches the smallest 16-bit displacement d that drops all its keys into free slots (h2 + d * PH_MULT) & mask.
// Returns false if some bucket cannot be placed (caller retries with another seed / a larger table).
bool chd_place(const std::vector<uint32_t>& h1, const std::vector<uint32_t>& h2, uint32_t mask, uint32_t bmask,
               std::vector<uint16_t>* disp, std::vector<uint32_t>* slot_of_key) {
    const uint32_t nb = bmask + 1, n = (uint32_t)h1.size();
    std::vector<std::vector<uint32_t>> buckets(nb);
    for (uint32_t i = 0; i < n; ++i) buckets[h1[i] & bmask].push_back(i);
    std::vector<uint32_t> order(nb);
    for (uint32_t b = 0; b < nb; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return buckets[x].size() > buckets[y].size(); });
    std::vector<uint8_t> used(mask + 1, 0);
    disp->assign(nb, 0);
    slot_of_key->assign(n, 0);
    std::vector<uint32_t> slots;
    for (uint32_t b : order) {
        const auto& keys = buckets[b];
        if (keys.empty()) break;
        bool placed = false;
        for (uint32_t d = 0; d < 65536 && !placed; ++d) {
            slots.clear();
            bool clash = false;
            for (uint32_t i : keys) {
                uint32_t sl = ph_slot(h2[i], d, mask);
                if (used[sl] || std::find(slots.begin(), slots.end(), sl) != slots.end()) { clash = true; break; }
                slots.push_back(sl);
            }
            if (!clash) {
                for (size_t k = 0; k < keys.size(); ++k) { used[slots[k]] = 1; (*slot_of_key)[keys[k]] = slots[k]; }
                (*disp)[b] = (uint16_t)d;
                placed = true;
            }
        }
        if (!placed) return false;
    }
    return true;
}

namespace {

struct UcRun {
    uint32_t first, last;
    uint8_t flags;
};
const UcRun kUcRuns[] = {
#include "unicode_ranges.inc"
};
const UcRun kUcCaseRuns[] = {      // (flags: UCC_UPPER / UCC_LOWER, tables.hpp)
#include "unicode_case_ranges.inc"
};
const UcRun kUcPsmRuns[] = {       // (flags: UC2_P / UC2_S / UC2_M / UC2_CJK, tables.hpp)
#include "unicode_psm_ranges.inc"
};
const UcRun kUcMarkRuns[] = {      // (flags: 1 = StripAccents removes the char)
#include "unicode_mark_ranges.inc"
};
const UcRun kUcNumericRuns[] = {   // (flags: UC_RUST_N, tables.hpp)
#include "unicode_numeric_ranges.inc"
};

const UcRun kGcRuns[] = {          // (flags: GC_* of precompiled_core.hpp)
#include "grapheme_tables.inc"
};

struct BnMapRow {
    uint32_t cp, a, b, c;
};
#define BN_WANT_RUNS
const UcRun kBnRuns[] = {
#include "bert_norm_tables.inc"
};
#undef BN_WANT_RUNS
#define BN_WANT_D
const BnMapRow kBnD[] = {
#include "bert_norm_tables.inc"
};
#undef BN_WANT_D
#define BN_WANT_LC
const BnMapRow kBnLC[] = {
#include "bert_norm_tables.inc"
};
#undef BN_WANT_LC
struct BnNfdRow {
    uint32_t cp, packed;
};
#define BN_WANT_NFD
const BnNfdRow kBnNFD[] = {
#include "bert_norm_tables.inc"
};
#undef BN_WANT_NFD
struct NfcDecompRow {
    uint32_t cp, d[4];
};
struct NfcCompRow {
    uint32_t a, b, c;
};
#define NFC_WANT_RUNS
const UcRun kNfcRuns[] = {
#include "nfc_tables.inc"
};
#undef NFC_WANT_RUNS
#define NFC_WANT_DECOMP
const NfcDecompRow kNfcDecomp[] = {
#include "nfc_tables.inc"
};
#undef NFC_WANT_DECOMP
#define NFC_WANT_COMP
const NfcCompRow kNfcComp[] = {
#include "nfc_tables.inc"
};
#undef NFC_WANT_COMP
struct NfkDecompRow {
    uint32_t cp, off, len;
};
#define NFKC_WANT_RUNS
const UcRun kNfkRuns[] = {
#include "nfkc_tables.inc"
};
#undef NFKC_WANT_RUNS
#define NFKC_WANT_DECOMP
const NfkDecompRow kNfkDecomp[] = {
#include "nfkc_tables.inc"
};
#undef NFKC_WANT_DECOMP
#define NFKC_WANT_FLAT
const uint32_t kNfkFlat[] = {
#include "nfkc_tables.inc"
};
#undef NFKC_WANT_FLAT

// GPT-2 bytes <-> unicode map, pre_tokenizers/byte_level.rs:15-39: printable bytes map to
// themselves, the other 68 bytes to U+0100+n in byte order.
void build_bytes_char(uint32_t b2c[256]) {
    bool direct[256] = {false};
    for (int b = '!'; b <= '~'; ++b) direct[b] = true;
    for (int b = 0xA1; b <= 0xAC; ++b) direct[b] = true;
    for (int b = 0xAE; b <= 0xFF; ++b) direct[b] = true;
    uint32_t n = 0;
    for (int b = 0; b < 256; ++b) {
        if (direct[b]) b2c[b] = (uint32_t)b;
        else b2c[b] = 256 + n++;
    }
}

// decode one UTF-8 scalar; returns length or 0 if malformed
int utf8_decode(const uint8_t* s, size_t n, uint32_t* cp) {
    if (n == 0) return 0;
    uint8_t b = s[0];
    if (b < 0x80) { *cp = b; return 1; }
    if ((b & 0xE0) == 0xC0 && n >= 2) { *cp = ((b & 0x1F) << 6) | (s[1] & 0x3F); return 2; }
    if ((b & 0xF0) == 0xE0 && n >= 3) { *cp = ((b & 0x0F) << 12) | ((s[1] & 0x3F) << 6) | (s[2] & 0x3F); return 3; }
    if ((b & 0xF8) == 0xF0 && n >= 4) {
        *cp = ((b & 0x07) << 18) | ((s[1] & 0x3F) << 12) | ((s[2] & 0x3F) << 6) | (s[3] & 0x3F);
        return 4;
    }
    return 0;
}

// token string in the byte-level alphabet -> raw bytes; false if a char is outside the alphabet
bool bytelevel_to_raw(const std::string& tok, const std::unordered_map<uint32_t, uint8_t>& c2b, std::string* raw) {
    raw->clear();
    const uint8_t* s = (const uint8_t*)tok.data();
    size_t n = tok.size(), i = 0;
    while (i < n) {
        uint32_t cp;
        int l = utf8_decode(s + i, n - i, &cp);
        if (!l) return false;
        auto it = c2b.find(cp);
        if (it == c2b.end()) return false;
        raw->push_back((char)it->second);
        i += l;
    }
    return true;
}

// a flag byte per code point -> the two stages the kernels index: the distinct 256-char blocks in order of first use, and per block its index
void two_stage(const std::vector<uint8_t>& flat, std::vector<uint16_t>* s1, std::vector<uint8_t>* s2) {
    s1->assign(UC_STAGE1_LEN, 0);
    s2->clear();
    std::unordered_map<std::string, uint16_t> seen;
    for (uint32_t blk = 0; blk < (uint32_t)UC_STAGE1_LEN; ++blk) {
        std::string key((const char*)&flat[blk * 256], 256);
        auto it = seen.find(key);
        if (it == seen.end()) {
            uint16_t idx = (uint16_t)(s2->size() / 256);
            s2->insert(s2->end(), key.begin(), key.end());
            it = seen.emplace(std::move(key), idx).first;
        }
        (*s1)[blk] = it->second;
    }
}

// the flags of a table of runs, one byte per code point
template <size_t N>
std::vector<uint8_t> flat_of(const UcRun (&runs)[N]) {
    std::vector<uint8_t> flat(0x110000, 0);
    for (const UcRun& r : runs)
        for (uint32_t cp = r.first; cp <= r.last; ++cp) flat[cp] = r.flags;
    return flat;
}

void build_unicode(HostModel& m) {
    std::vector<uint8_t> flat = flat_of(kUcRuns);
    // char::is_numeric, the class the Digits pre-tokenizer splits on: one more flag of the same byte, only where a kernel reads it
    if (m.pretok == PT_DIGITS_GPT2)
        for (const UcRun& r : kUcNumericRuns)
            for (uint32_t cp = r.first; cp <= r.last; ++cp) flat[cp] |= r.flags;
    // the 39 chars BLOOM's Split class leaves out, Oniguruma's \s and fourteen punctuation marks: the same bit, for this kind's handles only
    if (m.pretok == PT_BLOOM) {
        for (uint32_t cp = 0; cp < 0x110000u; ++cp)
            if (flat[cp] & UC_ONIG_S) flat[cp] |= UC_BLOOM_X;
        for (uint32_t cp : kBloomPunct) flat[cp] |= UC_BLOOM_X;
    }
    two_stage(flat, &m.uc_stage1, &m.uc_stage2);
}

template <class Slot, class IsEmpty, class H1, class H2>
bool cuckoo_insert(std::vector<Slot>& tab, Slot item, IsEmpty is_empty, H1 h1, H2 h2, std::mt19937& rng) {
    for (int kick = 0; kick < 2000; ++kick) {
        uint32_t s1 = h1(item), s2 = h2(item);
        if (is_empty(tab[s1])) { tab[s1] = item; return true; }
        if (is_empty(tab[s2])) { tab[s2] = item; return true; }
        uint32_t victim = (rng() & 1) ? s1 : s2;
        std::swap(item, tab[victim]);
    }
    return false;
}

void build_pair_table(const std::vector<MergeSlot>& items, std::vector<MergeSlot>* out, uint32_t* out_mask, uint32_t* out_seed) {
    if (items.empty()) { out->assign(16, MergeSlot{MERGE_EMPTY, MERGE_EMPTY, RANK_NONE, 0}); *out_mask = 15; *out_seed = 0; return; }
    uint32_t cap = 16;
    while (cap < items.size() * 5 / 2) cap <<= 1;   // load factor <= 0.4
    std::mt19937 rng(12345);
    for (int attempt = 0; attempt < 64; ++attempt) {
        uint32_t seed = (uint32_t)rng();
        uint32_t mask = cap - 1;
        std::vector<MergeSlot> tab(cap, MergeSlot{MERGE_EMPTY, MERGE_EMPTY, RANK_NONE, 0});
        bool ok = true;
        for (const MergeSlot& e : items) {
            ok = cuckoo_insert(
                tab, e, [](const MergeSlot& s) { return s.a == MERGE_EMPTY; },
                [&](const MergeSlot& s) { return merge_hash1(s.a, s.b, seed) & mask; },
                [&](const MergeSlot& s) { return merge_hash2(s.a, s.b, seed) & mask; }, rng);
            if (!ok) break;
        }
        if (ok) { out->swap(tab); *out_mask = mask; *out_seed = seed; return; }
        if (attempt % 4 == 3) cap <<= 1;
    }
    throw Invalid("could not build a pair hash table");
}

void build_merge_table(HostModel& m, const std::vector<MergeSlot>& merges) {
    // new_id == rank + constant for every merge (true of every trainer-produced vocabulary: merged tokens are
    // appended in merge order): the LDS-resident merge kernel then needs no per-pair new-id array
    m.merge_newid_affine = !merges.empty();
    m.merge_newid_base = merges.empty() ? 0u : merges[0].new_id - merges[0].rank;
    for (const MergeSlot& e : merges)
        if (e.new_id - e.rank != m.merge_newid_base) { m.merge_newid_affine = false; break; }
    uint32_t cap = 16;
    while (cap < merges.size() * 5 / 2) cap <<= 1;            // load factor <= 0.4
    uint32_t nb_wide = 16;
    while (nb_wide < merges.size() / 4) nb_wide <<= 1;        // 2-4 keys per bucket (50k merges -> 16384 buckets = 32 KB)
    // The merge kernels keep up to DISP_LDS_MAX displacements in LDS; beyond that every probe of the merge chain reads its
    // displacement from global memory first -- two dependent round trips instead of one (C4's 128 k merges: 32,768 buckets,
    // the merge kernels 0.17 ms against C2's 0.10).  More keys per bucket (8 at 128 k) only cost the builder trials: at load
    // factor <= 0.4 a bucket of k keys fits a given displacement with probability >= 0.6^k, and 16 bits of displacement are 65,536 tries.
    // (TKAMD_MERGE_BUCKETS=wide: the old sizing -- the tests' way to the global-displacement branch.)
    const char* wide_env = getenv("TKAMD_MERGE_BUCKETS");
    const bool want_wide = wide_env && !strcmp(wide_env, "wide");
    std::mt19937 rng(777);
    for (int attempt = 0; attempt < 32; ++attempt) {
        const uint32_t nb = (want_wide || attempt >= 8) ? nb_wide : std::min(nb_wide, (uint32_t)DISP_LDS_MAX);
        const uint32_t seed = (uint32_t)rng();
        std::vector<uint32_t> h1(merges.size()), h2(merges.size()), where;
        for (size_t i = 0; i < merges.size(); ++i) { h1[i] = merge_hash1(merges[i].a, merges[i].b, seed); h2[i] = merge_hash2(merges[i].a, merges[i].b, seed); }
        std::vector<uint16_t> disp;
        if (chd_place(h1, h2, cap - 1, nb - 1, &disp, &where)) {
            m.merge_table.assign(cap, MergeSlot{MERGE_EMPTY, MERGE_EMPTY, RANK_NONE, 0});
            for (size_t i = 0; i < merges.size(); ++i) m.merge_table[where[i]] = merges[i];
            m.merge_disp.swap(disp);
            m.merge_mask = cap - 1; m.merge_bmask = nb - 1; m.merge_seed = seed;
            return;
        }
        if (attempt % 8 == 7) cap <<= 1;                       // a new seed almost always does it; grow (at most 8x) only as a last resort
    }
    throw Invalid("could not build the merge hash table");
}

void build_word_table(HostModel& m, const std::vector<WordSlot>& words) {
    uint32_t cap = 16;
    while (cap < words.size() * 5 / 2) cap <<= 1;
    std::mt19937 rng(54321);
    for (int attempt = 0; attempt < 32; ++attempt) {
        const uint32_t seed = (uint32_t)rng();
        std::vector<uint32_t> h1(words.size()), tenant;
        for (size_t i = 0; i < words.size(); ++i) h1[i] = word_hash1(words[i].lo, words[i].hi, words[i].len, seed);
        if (cuckoo_place(h1, cap - 1, &tenant)) {
            m.word_table.assign(cap, WordSlot{0, 0, 0, 0, 0, 0});
            for (uint32_t sidx = 0; sidx < cap; ++sidx)
                if (tenant[sidx] != 0xFFFFFFFFu) m.word_table[sidx] = words[tenant[sidx]];
            m.word_mask = cap - 1; m.word_seed = seed;
            return;
        }
        if (attempt % 8 == 7) cap <<= 1;                          // a new seed almost always does it; grow only as a last resort
    }
    throw Invalid("could not build the whole-word hash table");
}

void build_long_table(HostModel& m) {
    size_t n = m.long_id.size();
    uint32_t cap = 16;
    while (cap < n * 2 + 1) cap <<= 1;
    m.long_mask = cap - 1;
    m.long_table.assign(cap, 0);
    for (size_t e = 0; e < n; ++e) {
        uint32_t h = fnv1a(&m.long_blob[m.long_off[e]], m.long_off[e + 1] - m.long_off[e]) & m.long_mask;
        while (m.long_table[h]) h = (h + 1) & m.long_mask;
        m.long_table[h] = (uint32_t)e + 1;
    }
}

// Build the two-root byte trie for WordPiece and flatten it into a cuckoo table.
void build_trie(HostModel& m, const std::vector<std::pair<std::string, uint32_t>>& initial,
                const std::vector<std::pair<std::string, uint32_t>>& cont) {
    struct Node {
        std::unordered_map<uint8_t, uint32_t> kids;
        uint32_t id = 0xFFFFFFFFu;
    };
    std::vector<Node> nodes(2);
    auto insert = [&](uint32_t root, const std::string& key, uint32_t id) {
        uint32_t cur = root;
        for (unsigned char c : key) {
            auto it = nodes[cur].kids.find(c);
            uint32_t nxt;
            if (it == nodes[cur].kids.end()) {
                nxt = (uint32_t)nodes.size();
                nodes.emplace_back();
                nodes[cur].kids.emplace(c, nxt);
            } else nxt = it->second;
            cur = nxt;
        }
        nodes[cur].id = id;
    };
    for (auto& kv : initial) insert(0, kv.first, kv.second);
    for (auto& kv : cont) insert(1, kv.first, kv.second);
    std::vector<MergeSlot> items;
    for (uint32_t n = 0; n < nodes.size(); ++n)
        for (auto& e : nodes[n].kids) items.push_back(MergeSlot{n, (uint32_t)e.first, e.second, nodes[e.second].id});
    if (nodes.size() >= ((size_t)1 << 24)) throw Unsupported("byte trie of the vocabulary (WordPiece / Unigram) beyond 2^24 nodes");
    m.trie.n_nodes = (uint32_t)nodes.size();
    build_pair_table(items, &m.trie.table, &m.trie.mask, &m.trie.seed);
}

// the members a normalizer chain is made of (tables.hpp ChainMember); -1: not one of them
int chain_member(const std::string& type) { return type == "NFD" ? CHAIN_NFD : type == "Lowercase" ? CHAIN_LOWERCASE : type == "StripAccents" ? CHAIN_STRIP_ACCENTS : -1; }
// a chain that reads well but stands in front of something it is not built for: refused in the words the section was always refused by
std::string chain_refusal(const HostModel& m, const std::string& what) {
    return "normalizer: " + m.chain_spelling + " is outside the hot path in front of " + what + " (NFD / Lowercase / StripAccents are on it in front of WordPiece, "
           "WordLevel and BPE over characters, behind Whitespace, WhitespaceSplit or BertPreTokenizer)";
}

// BertNormalizer data: flags as a 2-stage table, the NFD+strip (kind 0) and lowercase (kind 1) maps as one
// cuckoo table keyed (cp, kind) with the up-to-3 output code points packed 21 bits each
void build_bert_norm(HostModel& m) {
    two_stage(flat_of(kBnRuns), &m.bn_stage1, &m.bn_stage2);
    std::vector<MergeSlot> items;
    auto add = [&](const BnMapRow& r, uint32_t kind) {
        uint64_t v = (uint64_t)r.a | ((uint64_t)r.b << 21) | ((uint64_t)r.c << 42);
        items.push_back(MergeSlot{r.cp, kind, (uint32_t)v, (uint32_t)(v >> 32)});
    };
    for (const BnMapRow& r : kBnD) add(r, 0);
    for (const BnMapRow& r : kBnLC) add(r, 1);
    for (const BnNfdRow& r : kBnNFD) items.push_back(MergeSlot{r.cp, 2u, r.packed, 0u});      // kind 2: classes of the NFD pieces (bert_norm_core.hpp)
    build_pair_table(items, &m.bn_map, &m.bn_mask, &m.bn_seed);
}

// NORM_CHAIN data: every member is a map of single chars (NFD: the full canonical decomposition, nfc_tables.inc; Lowercase:
// char::to_lowercase, the kind-1 rows of bert_norm_tables.inc; StripAccents: drop the marks of unicode_mark_ranges.inc), and with
// StripAccents behind NFD nothing NFD's canonical ordering could move is left (tools/gen_mark_tables.py asserts it of the wheel), so the
// chain is the composition of its members per SOURCE char.  Composed here for every scalar: flag 1 on each char the chain changes, its
// expansion (<= 3 code points, 0x1FFFFF-filled; none: the char disappears) in the cuckoo table under (cp, 0) -- the BertNormalizer's layout.
void build_norm_chain(HostModel& m, const std::vector<uint8_t>& members) {
    constexpr uint32_t FILL = 0x1FFFFFu, S_BASE = 0xAC00u, S_N = 11172u;
    std::vector<uint8_t> prim(0x110000, 0);                   // 1 decomposes (table), 2 lowercases, 4 a mark
    std::unordered_map<uint32_t, const NfcDecompRow*> dec;
    std::unordered_map<uint32_t, const BnMapRow*> lc;
    for (const NfcDecompRow& r : kNfcDecomp) { dec[r.cp] = &r; prim[r.cp] |= 1; }
    for (const BnMapRow& r : kBnLC) { lc[r.cp] = &r; prim[r.cp] |= 2; }
    for (const UcRun& r : kUcMarkRuns)
        for (uint32_t cp = r.first; cp <= r.last; ++cp) prim[cp] |= 4;
    std::vector<uint8_t> flat(0x110000, 0);
    std::vector<MergeSlot> items;
    std::vector<uint32_t> cur, nxt;
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) {
        if (cp >= 0xD800u && cp < 0xE000u) continue;
        if (!prim[cp] && !(cp - S_BASE < S_N)) continue;      // no member touches it
        cur.assign(1, cp);
        for (uint8_t member : members) {
            nxt.clear();
            for (uint32_t c : cur) {
                if (member == CHAIN_NFD && c - S_BASE < S_N) {              // Hangul syllables: arithmetic
                    const uint32_t s = c - S_BASE;
                    nxt.push_back(0x1100u + s / 588u);
                    nxt.push_back(0x1161u + (s % 588u) / 28u);
                    if (s % 28u) nxt.push_back(0x11A7u + s % 28u);
                } else if (member == CHAIN_NFD && (prim[c] & 1)) {
                    for (uint32_t d : dec[c]->d) if (d != FILL) nxt.push_back(d);
                } else if (member == CHAIN_LOWERCASE && (prim[c] & 2)) {
                    const BnMapRow& r = *lc[c];
                    for (uint32_t d : {r.a, r.b, r.c}) if (d != FILL) nxt.push_back(d);
                } else if (member == CHAIN_STRIP_ACCENTS && (prim[c] & 4)) {
                } else nxt.push_back(c);
            }
            cur.swap(nxt);
        }
        if (cur.size() == 1 && cur[0] == cp) continue;
        uint32_t ob = 0;                                          // (the X text is bounded by three times the input, a lane's output by 7 bits)
        for (uint32_t c : cur) ob += bn_core_utf8_len(c);
        if (ob > 3u * bn_core_utf8_len(cp)) throw Invalid("normalizer chain: code point " + std::to_string(cp) + " grows more than three times in UTF-8");
        if (cur.size() > 3) throw Invalid("normalizer chain: code point " + std::to_string(cp) + " expands to more than three code points");
        cur.resize(3, FILL);
        const uint64_t v = (uint64_t)cur[0] | ((uint64_t)cur[1] << 21) | ((uint64_t)cur[2] << 42);
        items.push_back(MergeSlot{cp, 0u, (uint32_t)v, (uint32_t)(v >> 32)});
        flat[cp] = 1;
    }
    two_stage(flat, &m.bn_stage1, &m.bn_stage2);
    build_pair_table(items, &m.bn_map, &m.bn_mask, &m.bn_seed);
}

// NFC data: flags as a 2-stage table; one pair table with the full canonical decompositions -- (cp, 0) -> three code points packed 21
// bits each, (cp, 1) -> the fourth -- and the primary composites (first, second) -> composite (a second is never below U+0300)
void build_nfc_tables(HostModel& m) {
    two_stage(flat_of(kNfcRuns), &m.nfc_stage1, &m.nfc_stage2);
    std::vector<MergeSlot> items;
    for (const NfcDecompRow& r : kNfcDecomp) {
        const uint64_t v = (uint64_t)r.d[0] | ((uint64_t)r.d[1] << 21) | ((uint64_t)r.d[2] << 42);
        items.push_back(MergeSlot{r.cp, 0u, (uint32_t)v, (uint32_t)(v >> 32)});
        if (r.d[3] != NFC_FILL) items.push_back(MergeSlot{r.cp, 1u, r.d[3], 0u});
    }
    for (const NfcCompRow& r : kNfcComp) items.push_back(MergeSlot{r.a, r.b, r.c, 0u});
    build_pair_table(items, &m.nfc_map, &m.nfc_mask, &m.nfc_seed);
}

// K mode data (nfkc_tables.inc): the K flags in the flag table's place, NFC's pair table for the primary composites, and the full
// compatibility decompositions as one flat array behind a pair table (cp, 0) -> (offset, length)
void build_nfkc_tables(HostModel& m) {
    build_nfc_tables(m);
    two_stage(flat_of(kNfkRuns), &m.nfc_stage1, &m.nfc_stage2);
    m.nfk_flat.assign(kNfkFlat, kNfkFlat + NFKC_N_FLAT);
    std::vector<MergeSlot> items;
    for (const NfkDecompRow& r : kNfkDecomp) {
        if (r.len == 0u || r.len > (uint32_t)NFKC_MAX_DECOMP || (size_t)r.off + r.len > m.nfk_flat.size()) throw Invalid("nfkc_tables.inc: a decomposition outside the flat array");
        items.push_back(MergeSlot{r.cp, 0u, r.off, r.len});
    }
    build_pair_table(items, &m.nfk_map, &m.nfk_mask, &m.nfk_seed);
}

// The top-level alternatives of a regex source: cut at every '|' outside (...) and [...]; a backslash escapes the next character.
std::vector<std::string> regex_alternatives(const std::string& rx) {
    std::vector<std::string> out(1);
    int depth = 0;
    bool cls = false;
    for (size_t i = 0; i < rx.size(); ++i) {
        const char c = rx[i];
        if (c == '\\' && i + 1 < rx.size()) { out.back() += c; out.back() += rx[++i]; continue; }
        if (cls) { if (c == ']') cls = false; }
        else if (c == '[') cls = true;
        else if (c == '(') ++depth;
        else if (c == ')') --depth;
        else if (c == '|' && depth == 0) { out.emplace_back(); continue; }
        out.back() += c;
    }
    return out;
}

// Split(Regex(pattern), Isolated) of the tiktoken family -> the parameters of tables.hpp SplitRule (pre_tokenizers/split.rs:76-105 hands
// the pattern to Oniguruma, tokenizer/pattern.rs:63-83; here the pattern is READ, alternative by alternative, and everything that is not
// one of the family's spellings is refused).  *gpt2: the pattern is the GPT-2 regex itself (byte_level.rs:43-46), served by that kernel.
bool parse_split_pattern(const std::string& rx, SplitRule* rule, bool* gpt2, std::string* why) {
    *gpt2 = rx == "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    if (*gpt2) return true;
    const std::vector<std::string> alt = regex_alternatives(rx);
    size_t k = 0;
    SplitRule r{0, 0, 3, 1};
    static const char* const lits[7] = {"'s", "'t", "'re", "'ve", "'m", "'ll", "'d"};
    const std::string ci = "(?i:'s|'t|'re|'ve|'m|'ll|'d)";
    auto at = [&](size_t i) -> const std::string& { static const std::string none; return i < alt.size() ? alt[i] : none; };
    if (at(k) == ci || at(k) == "'(?i:[sdmt]|ll|ve|re)") { r.contr = 1; ++k; }
    else {
        bool all = alt.size() >= 7;
        for (size_t q = 0; q < 7 && all; ++q) all = alt[q] == lits[q];
        if (all) { r.contr = 2; k = 7; }
    }
    const std::string pre = "[^\\r\\n\\p{L}\\p{N}]?", up = "[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]", lo = "[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]";
    if (at(k) == pre + "\\p{L}+") { r.letters = 0; ++k; }
    else if ((at(k) == pre + up + "*" + lo + "+" && at(k + 1) == pre + up + "+" + lo + "*") ||
             (at(k) == pre + up + "*" + lo + "+" + ci + "?" && at(k + 1) == pre + up + "+" + lo + "*" + ci + "?")) {
        if (at(k).size() > (pre + up + "*" + lo + "+").size()) {
            if (r.contr) { *why = "contractions both as an alternative and as a suffix of the letter alternatives"; return false; }
            r.contr = 3;
        }
        r.letters = 2;
        k += 2;
    } else { *why = "letter alternative '" + at(k) + "'"; return false; }
    if (at(k) == "\\p{N}{1,3}") r.digit_max = 3;
    else if (at(k) == "\\p{N}{1,2}") r.digit_max = 2;
    else if (at(k) == "\\p{N}" || at(k) == "\\p{N}{1}" || at(k) == "\\p{N}{1,1}") r.digit_max = 1;
    else if (at(k) == "\\p{N}+") r.digit_max = 0;
    else { *why = "digit alternative '" + at(k) + "'"; return false; }
    ++k;
    if (at(k) == " ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*") r.other_tail = 1;
    else if (at(k) == " ?[^\\s\\p{L}\\p{N}]+[\\r\\n/]*") r.other_tail = 2;
    else { *why = "alternative '" + at(k) + "'"; return false; }
    ++k;
    if (at(k) != "\\s*[\\r\\n]+" || at(k + 1) != "\\s+(?!\\S)" || at(k + 2) != "\\s+" || alt.size() != k + 3) {
        *why = "the whitespace alternatives are not \\s*[\\r\\n]+|\\s+(?!\\S)|\\s+";
        return false;
    }
    *rule = r;
    return true;
}

// ---- the DeepSeek-V3 chain: Sequence[Split(\p{N}{1,3}), Split([CJK class]+), Split(stage 3), ByteLevel(use_regex=false)] -------------------
// (pretok_ds3_core.hpp).  The three patterns are READ like the tiktoken family's: alternative by alternative, the two classes the rule
// depends on by their MEMBER SETS, whatever the spelling.

std::string cp_name(uint32_t cp) {
    char buf[16];
    snprintf(buf, sizeof buf, "U+%04X", cp);
    return buf;
}

// A bracket class of literal members at rx[*pos] == '[': chars, ranges a-b, backslash escapes of punctuation, \r \n \t, \xHH, \uHHHH,
// \x{H..}.  The members go to *out and *pos behind the ']'.  False (with *why) for a negated class or one that holds a property or a nested class.
bool parse_literal_class(const std::string& rx, size_t* pos, std::set<uint32_t>* out, std::string* why) {
    const uint8_t* s = (const uint8_t*)rx.data();
    const size_t n = rx.size();
    size_t i = *pos;
    if (i >= n || s[i] != '[') { *why = "a bracket class was expected in '" + rx + "'"; return false; }
    ++i;
    if (i < n && s[i] == '^') { *why = "negated class in '" + rx + "'"; return false; }
    auto member = [&](uint32_t* cp) -> bool {            // one member at i
        if (s[i] == '\\') {
            if (i + 1 >= n) return false;
            const char e = (char)s[i + 1];
            i += 2;
            if (e == 'r') { *cp = '\r'; return true; }
            if (e == 'n') { *cp = '\n'; return true; }
            if (e == 't') { *cp = '\t'; return true; }
            if (e == 'x' || e == 'u') {
                size_t digits = e == 'u' ? 4 : 2;
                bool braces = i < n && s[i] == '{';
                if (braces) { ++i; digits = 8; }
                uint32_t v = 0;
                size_t k = 0;
                for (; k < digits && i < n && isxdigit(s[i]); ++k, ++i) v = v * 16 + (uint32_t)(isdigit(s[i]) ? s[i] - '0' : (s[i] | 0x20) - 'a' + 10);
                if (k == 0 || (!braces && k != digits)) return false;
                if (braces) { if (i >= n || s[i] != '}') return false; ++i; }
                *cp = v;
                return true;
            }
            if (isalnum((unsigned char)e)) return false;   // \p{..}, \s, \d, \w ...: not a literal member
            *cp = (uint8_t)e;
            return true;
        }
        if (s[i] == '[') return false;
        const int l = utf8_decode(s + i, n - i, cp);
        if (!l) return false;
        i += l;
        return true;
    };
    bool first = true;
    while (i < n && (s[i] != ']' || first)) {
        first = false;
        uint32_t a, b;
        if (!member(&a)) { *why = "a class member that is not a literal char in '" + rx + "'"; return false; }
        b = a;
        if (i + 1 < n && s[i] == '-' && s[i + 1] != ']') {
            ++i;
            if (!member(&b) || b < a) { *why = "a bad range in '" + rx + "'"; return false; }
        }
        if (b - a > 0x10000u) { *why = "a range of more than 65,536 chars in '" + rx + "'"; return false; }
        for (uint32_t c = a; c <= b; ++c) out->insert(c);
    }
    if (i >= n) { *why = "unterminated class in '" + rx + "'"; return false; }
    *pos = i + 1;
    return true;
}

// `got` against `want`: the first member one of them has and the other lacks, named
bool same_members(const std::set<uint32_t>& got, const std::set<uint32_t>& want, const char* what, std::string* why) {
    for (uint32_t c : got)
        if (!want.count(c)) { *why = std::string(what) + " holds " + cp_name(c) + ", which is not in the class the path builds"; return false; }
    for (uint32_t c : want)
        if (!got.count(c)) { *why = std::string(what) + " lacks " + cp_name(c); return false; }
    return true;
}

// raw CR / LF / TAB in a pattern (JSON decodes "\r" to the char itself) -> their escapes, so both spellings read alike
std::string escape_controls(const std::string& rx) {
    std::string o;
    for (char c : rx) {
        if (c == '\r') o += "\\r";
        else if (c == '\n') o += "\\n";
        else if (c == '\t') o += "\\t";
        else o += c;
    }
    return o;
}

enum ChainStage { CHAIN_DIGITS = 1, CHAIN_CJK = 2, CHAIN_MAIN = 3 };
// which stage a pattern is meant to be (by its outline; the stage's own reader then accepts or refuses it)
ChainStage chain_stage_of(const std::string& rx) {
    if (rx.compare(0, 5, "\\p{N}") == 0 && rx.find('|') == std::string::npos) return CHAIN_DIGITS;
    if (!rx.empty() && rx[0] == '[' && rx.find('|') == std::string::npos && rx.find("\\p{") == std::string::npos) return CHAIN_CJK;
    return CHAIN_MAIN;
}

void parse_chain_digits(const std::string& rx) {
    if (rx != "\\p{N}{1,3}") throw Unsupported("pre_tokenizer: chained Split: digit count '" + rx + "' (only \\p{N}{1,3} is on the path)");
}

void parse_chain_cjk(const std::string& rx) {
    std::set<uint32_t> got, want;
    for (uint32_t c = 0x4E00; c <= 0x9FA5; ++c) want.insert(c);
    for (uint32_t c = 0x3040; c <= 0x30FF; ++c) want.insert(c);
    size_t pos = 0;
    std::string why;
    if (!parse_literal_class(rx, &pos, &got, &why)) throw Unsupported("pre_tokenizer: chained Split: CJK class: " + why);
    if (rx.compare(pos, std::string::npos, "+") != 0) throw Unsupported("pre_tokenizer: chained Split: CJK class: '" + rx + "' is not a class followed by +");
    if (!same_members(got, want, "the CJK class", &why))
        throw Unsupported("pre_tokenizer: chained Split: " + why + " (only [U+4E00-U+9FA5 U+3040-U+309F U+30A0-U+30FF]+ is on the path)");
}

void parse_chain_main(const std::string& rx_in) {
    const std::string rx = escape_controls(rx_in);
    const std::vector<std::string> alt = regex_alternatives(rx);
    const std::string head = "pre_tokenizer: chained Split: third pattern: ";
    if (alt.size() != 6) throw Unsupported(head + std::to_string(alt.size()) + " alternatives where the path builds six");
    {
        std::set<uint32_t> got, want;
        for (uint32_t c = 0x21; c < 0x7F; ++c)
            if (!isalnum((int)c)) want.insert(c);
        size_t pos = 0;
        std::string why;
        if (!parse_literal_class(alt[0], &pos, &got, &why)) throw Unsupported(head + "punctuation class: " + why);
        if (alt[0].compare(pos, std::string::npos, "[A-Za-z]+") != 0) throw Unsupported(head + "alternative '" + alt[0] + "' is not [punctuation][A-Za-z]+");
        if (!same_members(got, want, "the punctuation class", &why)) throw Unsupported(head + why + " (the 32 ASCII punctuation chars)");
    }
    static const char* const rest[5] = {"[^\\r\\n\\p{L}\\p{P}\\p{S}]?[\\p{L}\\p{M}]+", " ?[\\p{P}\\p{S}]+[\\r\\n]*", "\\s*[\\r\\n]+", "\\s+(?!\\S)", "\\s+"};
    for (int k = 0; k < 5; ++k)
        if (alt[k + 1] != rest[k]) throw Unsupported(head + "alternative '" + alt[k + 1] + "' where the path builds '" + rest[k] + "'");
}

// pt is a Sequence of more than two pre-tokenizers that ends in a ByteLevel and holds nothing but Splits in front of it
bool parse_split_chain(const JsonValue* seq, HostModel& m) {
    const size_t n = seq->arr.size();
    if (n < 3 || seq->arr[n - 1]->get_str("type") != "ByteLevel") return false;
    for (size_t k = 0; k + 1 < n; ++k)
        if (seq->arr[k]->get_str("type") != "Split") return false;
    if (n != 4) throw Unsupported("pre_tokenizer: a chain of " + std::to_string(n - 1) + " Splits in front of ByteLevel (only the chain of three -- digits, CJK class, "
                                  "main pattern -- is on the path)");
    std::string rx[3];
    for (size_t k = 0; k < 3; ++k) {
        const JsonValue* a = seq->arr[k].get();
        const JsonValue* pat = a->get("pattern");
        rx[k] = pat ? pat->get_str("Regex") : "";
        const bool invert = a->get_bool("invert", false);
        const std::string beh = a->get_str("behavior");
        if (rx[k].empty()) throw Unsupported("pre_tokenizer: chained Split with a String pattern (only Regex patterns are on the path)");
        if (invert || beh != "Isolated") throw Unsupported("pre_tokenizer: chained Split with behavior '" + beh + "'" + (invert ? " inverted" : "") + " (only Isolated is on the path)");
    }
    const JsonValue* b = seq->arr[3].get();
    if (b->get_bool("use_regex", true)) throw Unsupported("pre_tokenizer: Sequence[Split, Split, Split, ByteLevel(use_regex=true)] applies one regex more");
    if (b->get_bool("add_prefix_space", true))
        throw Unsupported("pre_tokenizer: Sequence[Split, Split, Split, ByteLevel(add_prefix_space=true)] (a prefix space in front of every pre-token)");
    const ChainStage got[3] = {chain_stage_of(rx[0]), chain_stage_of(rx[1]), chain_stage_of(rx[2])};
    if (got[0] != CHAIN_DIGITS || got[1] != CHAIN_CJK || got[2] != CHAIN_MAIN)
        throw Unsupported("pre_tokenizer: chained Split: the order of the stages is not digits, CJK class, main pattern");
    parse_chain_digits(rx[0]);
    parse_chain_cjk(rx[1]);
    parse_chain_main(rx[2]);
    m.byte_level = true;
    m.add_prefix_space = false;
    return true;
}

// ---- Sequence[Digits(individual_digits), ByteLevel(use_regex=true)]: StarCoder / StarCoder2 / SantaCoder, Granite code, Command-R --------
// (pretok_digits_core.hpp).  True for that Sequence; false for a Sequence that holds no Digits; every other place of a Digits is refused
// with its reason.
bool parse_digits_bytelevel(const JsonValue* seq, HostModel& m) {
    const size_t n = seq->arr.size();
    size_t at = n;
    for (size_t k = 0; k < n; ++k)
        if (seq->arr[k] && seq->arr[k]->get_str("type") == "Digits") { at = k; break; }
    if (at == n) return false;
    bool bytelevel_in_front = false;
    for (size_t k = 0; k < at; ++k) bytelevel_in_front |= seq->arr[k] && seq->arr[k]->get_str("type") == "ByteLevel";
    // behind ByteLevel the text is the byte-level alphabet, where six byte values (0xB2 0xB3 0xB9 0xBC 0xBD 0xBE) are numeric chars: Digits
    // then splits inside code points
    if (bytelevel_in_front)
        throw Unsupported("pre_tokenizer: this Sequence is outside the hot path: Digits behind ByteLevel reads the byte-level alphabet and splits inside code points "
                          "(Falcon's Sequence[Punctuation, ByteLevel, Digits, Split] chain)");
    if (n != 2 || at != 0)
        throw Unsupported("pre_tokenizer: this Sequence is outside the hot path: Digits in a chain of " + std::to_string(n) + " pre-tokenizers (Falcon's "
                          "Sequence[Punctuation, ByteLevel, Digits, Split] chain is one); only Sequence[Digits, ByteLevel] is on it");
    const JsonValue* b = seq->arr[1].get();
    if (!b || b->get_str("type") != "ByteLevel")
        throw Unsupported("pre_tokenizer: Sequence[Digits, " + (b ? b->get_str("type") : std::string("null")) + "]: only Sequence[Digits, ByteLevel] is on the path");
    if (!b->get_bool("use_regex", true))
        throw Unsupported("pre_tokenizer: Sequence[Digits, ByteLevel(use_regex=false)] is outside the hot path (only use_regex=true behind Digits is on it)");
    // ByteLevel::pre_tokenize puts its prefix space in front of every piece it is handed (byte_level.rs:122-125): behind Digits in front of
    // every digit
    if (b->get_bool("add_prefix_space", true))
        throw Unsupported("pre_tokenizer: Sequence[Digits, ByteLevel(add_prefix_space=true)] (a prefix space in front of every piece Digits cuts)");
    m.digits_individual = seq->arr[0]->get_bool("individual_digits", false);
    m.byte_level = true;
    m.add_prefix_space = false;
    return true;
}

const char* const kMetaspace = "\xE2\x96\x81";     // U+2581, the "▁" of SentencePiece
// the Split pattern of the CLIP files (CLIPTokenizerFast, the text encoders of Stable Diffusion / SDXL, the OpenCLIP conversions), byte for
// byte: with behavior Removed and invert = true its matches are the pre-tokens and the \s runs between them belong to none (pretok_clip_core.hpp)
const char* const kClipPattern = "'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+";
// BLOOM / BLOOMZ: " ?" and a run of the chars outside a class of 39 (pretok_bloom_core.hpp)
const char* const kBloomPattern = " ?[^(\\s|[.,!?…。，、।۔،])]+";

// A JSON number as serde_json reads it into an f64 WITHOUT its float_roundtrip feature -- how the reference is built (tokenizers/Cargo.toml:
// serde_json = "1.0", no features) and so what its Unigram scores are: the digits are gathered into a u64 significand (those that no
// longer fit are dropped), converted to f64 and multiplied or divided by ONE power of ten from a table (serde_json src/de.rs parse_integer,
// parse_decimal, parse_decimal_overflow, parse_long_integer, parse_exponent, f64_from_parts).  Two roundings where strtod makes one: 153 of
// the 3,000 seeded scores of tests/golden/unigram_ms come out one ulp off strtod's, and a Viterbi comparison can turn on that ulp.
double serde_json_f64(const std::string& t) {
    static const std::vector<double> pow10 = [] { std::vector<double> p; for (int e = 0; e <= 308; ++e) p.push_back(strtod(("1e" + std::to_string(e)).c_str(), nullptr)); return p; }();
    size_t i = 0;
    const size_t n = t.size();
    auto digit_at = [&](size_t k) { return k < n && t[k] >= '0' && t[k] <= '9'; };
    auto would_overflow = [](uint64_t a, uint64_t b) { const uint64_t c = ~0ull; return a >= c / 10 && (a > c / 10 || b > c % 10); };
    const bool positive = !(n && t[0] == '-');
    if (!positive) ++i;
    if (!digit_at(i)) throw Invalid("tokenizer.json: bad number '" + t + "'");
    uint64_t sig = 0;
    int32_t exponent = 0;
    bool is_float = false;
    if (t[i] == '0') ++i;
    else {
        while (digit_at(i)) {
            const uint64_t d = (uint64_t)(t[i] - '0');
            if (would_overflow(sig, d)) {                 // parse_long_integer: the digits that no longer fit only count
                is_float = true;
                while (digit_at(i)) { ++i; ++exponent; }
                break;
            }
            sig = sig * 10 + d;
            ++i;
        }
    }
    if (i < n && t[i] == '.') {
        is_float = true;
        ++i;
        if (!digit_at(i)) throw Invalid("tokenizer.json: bad number '" + t + "'");
        while (digit_at(i)) {
            const uint64_t d = (uint64_t)(t[i] - '0');
            if (would_overflow(sig, d)) {                 // parse_decimal_overflow: "just ignore all further digits"
                while (digit_at(i)) ++i;
                break;
            }
            sig = sig * 10 + d;
            --exponent;
            ++i;
        }
    }
    if (i < n && (t[i] == 'e' || t[i] == 'E')) {
        is_float = true;
        ++i;
        bool pos_exp = true;
        if (i < n && (t[i] == '+' || t[i] == '-')) { pos_exp = t[i] == '+'; ++i; }
        if (!digit_at(i)) throw Invalid("tokenizer.json: bad number '" + t + "'");
        int64_t ex = 0;
        bool huge = false;
        while (digit_at(i)) { ex = ex * 10 + (t[i] - '0'); if (ex > 0x7FFFFFFFll) { huge = true; ex = 0x7FFFFFFFll; } ++i; }
        if (huge) {                                       // parse_exponent_overflow
            if (sig != 0 && pos_exp) throw Invalid("tokenizer.json: number out of range '" + t + "'");
            return positive ? 0.0 : -0.0;
        }
        const int64_t fe = pos_exp ? (int64_t)exponent + ex : (int64_t)exponent - ex;
        exponent = (int32_t)std::max<int64_t>(std::min<int64_t>(fe, 0x7FFFFFFFll), -0x80000000ll);
    }
    if (i != n) throw Invalid("tokenizer.json: bad number '" + t + "'");
    if (!is_float) {
        // an integer: u64, or i64 when negative and in range; `as f64` rounds to nearest
        if (positive) return (double)sig;
        const int64_t neg = (int64_t)(0ull - sig);
        return neg >= 0 ? -(double)sig : (double)neg;
    }
    double f = (double)sig;                               // f64_from_parts
    for (;;) {
        const uint32_t a = exponent < 0 ? (uint32_t)(-(int64_t)exponent) : (uint32_t)exponent;
        if (a < pow10.size()) {
            if (exponent >= 0) {
                f *= pow10[a];
                if (std::isinf(f)) throw Invalid("tokenizer.json: number out of range '" + t + "'");
            } else f /= pow10[a];
            break;
        }
        if (f == 0.0) break;
        if (exponent >= 0) throw Invalid("tokenizer.json: number out of range '" + t + "'");
        f /= 1e308;
        exponent += 308;
    }
    return positive ? f : -f;
}

bool base64_decode(const std::string& in, std::string* out) {
    uint32_t acc = 0;
    int bits = 0;
    size_t pad = 0;
    for (char ch : in) {
        int v;
        if (ch >= 'A' && ch <= 'Z') v = ch - 'A';
        else if (ch >= 'a' && ch <= 'z') v = ch - 'a' + 26;
        else if (ch >= '0' && ch <= '9') v = ch - '0' + 52;
        else if (ch == '+' || ch == '-') v = 62;
        else if (ch == '/' || ch == '_') v = 63;
        else if (ch == '=') { ++pad; continue; }
        else if (ch == '\n' || ch == '\r') continue;
        else return false;
        if (pad) return false;
        acc = (acc << 6) | (uint32_t)v;
        bits += 6;
        if (bits >= 8) { bits -= 8; out->push_back((char)((acc >> bits) & 0xFFu)); }
    }
    return pad <= 2;
}

// ---- small readers of the tokenizer.json sections ----
// the array a Sequence section keeps its members under ("normalizers", "pretokenizers", "processors"), or null
const JsonValue* members_of(const JsonValue* section, const char* key) {
    const JsonValue* a = section ? section->get(key) : nullptr;
    return (a && a->is_array()) ? a : nullptr;
}
// the type of a section or of a Sequence's member; `other` for what is no object
std::string member_type(const JsonValue* v, const char* other = "?") { return (v && v->is_object()) ? v->get_str("type") : other; }
// how a refusal names the file's pre-tokenizer
std::string type_name_or_null(const JsonValue* pt) { return member_type(pt, "null"); }
// a Metaspace's prepend scheme, where it stands alone and behind WhitespaceSplit (pre_tokenizers/metaspace.rs:34-77: the legacy
// add_prefix_space = false means "never"); only the U+2581 replacement is on the path
std::string metaspace_scheme(const JsonValue* ms) {
    const std::string rep = ms->get_str("replacement");
    if (rep != kMetaspace) throw Unsupported("pre_tokenizer: Metaspace with replacement '" + rep + "' (only U+2581 is on the path)");
    const JsonValue* ps = ms->get("prepend_scheme");
    return (ps && ps->is_string()) ? ps->str : (ms->get_bool("add_prefix_space", true) ? "always" : "never");
}

// Sequence[Split(a), ByteLevel(b)]: the CLIP layout, BLOOM's, or a member of the tiktoken family -- in this order, each behind its own refusals
PretokKind parse_split_bytelevel(const JsonValue* a, const JsonValue* b, HostModel& m) {
    const JsonValue* pat = a->get("pattern");
    std::string rx = pat ? pat->get_str("Regex") : "";
    bool invert = a->get_bool("invert", false);
    std::string beh = a->get_str("behavior");
    m.byte_level = true;                 // (every layout accepted below is byte-level, without a prefix space)
    m.add_prefix_space = false;
    if (rx.empty()) throw Unsupported("pre_tokenizer: Split with a String pattern (only Regex patterns of the tiktoken family are on the path)");
    if (rx == kClipPattern) {
        // the CLIP layout.  ByteLevel's own regex (use_regex = true, as the files have it) matches every piece this pattern can cut
        // as one whole, so both spellings of use_regex are the same pre-tokenizer
        if (!invert || beh != "Removed")
            throw Unsupported("pre_tokenizer: the CLIP Split pattern with behavior '" + beh + "'" + (invert ? " inverted" : ", not inverted") +
                              " (only Removed, inverted, is on the path: the pattern's matches are the pre-tokens)");
        if (b->get_bool("add_prefix_space", true))
            throw Unsupported("pre_tokenizer: Sequence[Split(the CLIP pattern), ByteLevel(add_prefix_space=true)] (a prefix space in front of every pre-token)");
        if (!m.nfc_lower)
            throw Unsupported("pre_tokenizer: the CLIP Split is only on the path behind the normalizer Sequence[NFC, Replace(Regex '\\s+' -> ' '), Lowercase] "
                              "(with or without the Replace)");
        return PT_CLIP;
    }
    if (invert && beh == "Removed")
        throw Unsupported("pre_tokenizer: Split with behavior 'Removed' inverted (only Isolated is on the path; Removed, inverted, with the CLIP pattern alone, "
                          "which this pattern is not)");
    if (invert || beh != "Isolated") throw Unsupported("pre_tokenizer: Split with behavior '" + beh + "'" + (invert ? " inverted" : "") + " (only Isolated is on the path)");
    if (b->get_bool("use_regex", true)) throw Unsupported("pre_tokenizer: Sequence[Split, ByteLevel(use_regex=true)] applies two regexes");
    // ByteLevel::pre_tokenize puts its prefix space in front of every SPLIT it is handed (byte_level.rs:122-125) -- behind a Split
    // that is every pre-token, not every document: no tokenizer in use is configured that way, and the path does not build it
    if (b->get_bool("add_prefix_space", true))
        throw Unsupported("pre_tokenizer: Sequence[Split, ByteLevel(add_prefix_space=true)] (a prefix space in front of every pre-token)");
    if (rx == kBloomPattern) {
        // the BLOOM layout, by the exact pattern string (a pattern one char off is read by the family's parser below and refused
        // there); Isolated, not inverted, use_regex=false and no prefix space are established above
        if (m.norm != NORM_NONE)
            throw Unsupported("pre_tokenizer: BLOOM's Split + ByteLevel behind a normalizer is outside the hot path (only normalizer: null is on it)");
        return PT_BLOOM;
    }
    SplitRule rule{};
    bool gpt2 = false;
    std::string why;
    if (!parse_split_pattern(rx, &rule, &gpt2, &why))
        throw Unsupported("pre_tokenizer: Split pattern outside the tiktoken family (" + why + ")");
    if (gpt2) return PT_BYTELEVEL_GPT2;
    m.split_rule = rule;
    return PT_LLAMA3;
}

// reads "pre_tokenizer", norm, nfc_lower, pc_space_runs; writes byte_level, add_prefix_space, ms_*, split_rule, digits_individual and returns
// the kind.  A pre-tokenizer refuses HERE the normalizers it does not stand behind; what follows from the kind is finish_pretok's.
PretokKind parse_pretok(const JsonValue* pt, HostModel& m) {
    if (!pt || pt->is_null()) {
        // the "▁" normalizers leave every piece ONE pre-token (the device cuts it into units: the model check below proves that exact)
        if (m.norm == NORM_METASPACE) return PT_METASPACE;
        throw Unsupported("pre_tokenizer: null is outside the hot path");
    }
    std::string type = pt->get_str("type");
    if (type == "Split") {
        // Gemma-2 / Gemma-3: Split(String " ", MergedWithPrevious) behind Replace(" " -> "▁").  The normalizer leaves no space to split at,
        // so the Split is inert and the layout is the "▁" front with a null pre-tokenizer (the whole-piece checks of the model below stay in
        // force).  Inverted it is not inert -- the whole text is one match -- and nothing else about it is taken on trust.
        if (m.norm != NORM_METASPACE)
            throw Unsupported("pre_tokenizer: Split alone is outside the hot path (only Split(String ' ', MergedWithPrevious) behind the U+2581 normalizers, "
                              "where it is inert, is on it; and the Splits of Sequence[Split, ByteLevel])");
        const JsonValue* pat = pt->get("pattern");
        const JsonValue* lit = pat ? pat->get("String") : nullptr;
        if (!lit || !lit->is_string())
            throw Unsupported("pre_tokenizer: Split with a Regex pattern behind the U+2581 normalizers (only the String ' ', which they leave no match for, is on the path)");
        if (lit->str != " ")
            throw Unsupported("pre_tokenizer: Split with the String pattern '" + lit->str + "' behind the U+2581 normalizers (only the String ' ', which they leave no match for, "
                              "is on the path)");
        const std::string beh = pt->get_str("behavior");
        if (beh != "MergedWithPrevious")
            throw Unsupported("pre_tokenizer: Split(String ' ') with behavior '" + beh + "' behind the U+2581 normalizers (only MergedWithPrevious is on the path)");
        if (pt->get_bool("invert", false))
            throw Unsupported("pre_tokenizer: Split(String ' ') with invert = true behind the U+2581 normalizers (inverted, the whole text is one match: not inert)");
        return PT_METASPACE;
    }
    // (the U+2581 normalizers are the front of SentencePiece conversions: in front of any pre-tokenizer but none they are outside the path)
    if (m.norm == NORM_METASPACE && type != "Metaspace")
        throw Unsupported("normalizer: the U+2581 normalizers (Prepend / Replace ' ' -> U+2581) in front of pre_tokenizer '" + type +
                          "' are outside the hot path (only with a null pre_tokenizer)");
    if (type == "Metaspace") {
        // pre_tokenizers/metaspace.rs:34-77 (deserialisation: split defaults to true, the legacy add_prefix_space = false means "never")
        if (m.norm != NORM_NONE && m.norm != NORM_PRECOMPILED && m.norm != NORM_NFKC) throw Unsupported("pre_tokenizer: Metaspace behind a normalizer");
        // (behind bare Metaspace a run of spaces is a run of U+2581: the Replace(Regex " {2,}") member is not inert there)
        if (m.pc_space_runs) throw Unsupported("normalizer: Replace(Regex ' {2,}' -> ' ') behind Precompiled is only on the path in front of Sequence[WhitespaceSplit, Metaspace]");
        const std::string scheme = metaspace_scheme(pt);
        if (scheme == "always") m.ms_prepend = MS_ALWAYS;
        else if (scheme == "first") m.ms_prepend = MS_FIRST;
        else if (scheme == "never") m.ms_prepend = MS_NEVER;
        else throw Invalid("tokenizer.json: Metaspace prepend_scheme '" + scheme + "'");
        m.ms_split = pt->get_bool("split", true);
        return PT_METASPACE;
    }
    if (type == "ByteLevel") {
        m.byte_level = true;
        m.add_prefix_space = pt->get_bool("add_prefix_space", true);
        bool use_regex = pt->get_bool("use_regex", true);
        return use_regex ? PT_BYTELEVEL_GPT2 : PT_BYTELEVEL_NOREGEX;
    }
    if (type == "Whitespace") return PT_WHITESPACE;
    if (type == "WhitespaceSplit") return PT_WHITESPACE_SPLIT;
    if (type == "BertPreTokenizer") return PT_BERT;
    if (type == "Digits") throw Unsupported("pre_tokenizer: Digits alone is outside the hot path (only Sequence[Digits, ByteLevel] in front of byte-level BPE is on it)");
    if (type == "Sequence") {
        const JsonValue* seq = members_of(pt, "pretokenizers");
        if (seq && seq->arr.size() == 2 && seq->arr[0]->get_str("type") == "Split" && seq->arr[1]->get_str("type") == "ByteLevel")
            return parse_split_bytelevel(seq->arr[0].get(), seq->arr[1].get(), m);
        if (seq && seq->arr.size() == 2 && seq->arr[0] && seq->arr[1] && seq->arr[0]->get_str("type") == "WhitespaceSplit" &&
            seq->arr[1]->get_str("type") == "Metaspace") {
            // Sequence[WhitespaceSplit, Metaspace] (XLM-R, T5, mBART): the words between char::is_whitespace chars, each with its "▁".  On the
            // path behind Precompiled alone: the front then reads the normalizer's text, where the word rule runs (kernels/metaspace.hip MS_WORD)
            if (m.norm != NORM_PRECOMPILED)
                throw Unsupported("pre_tokenizer: Sequence[WhitespaceSplit, Metaspace] is only on the path behind a Precompiled normalizer");
            const JsonValue* b = seq->arr[1].get();
            const std::string scheme = metaspace_scheme(b);
            if (scheme != "always")
                throw Unsupported("pre_tokenizer: Sequence[WhitespaceSplit, Metaspace] with prepend_scheme '" + scheme + "' (only 'always' is on the path)");
            m.ms_prepend = MS_WORD;
            m.ms_split = b->get_bool("split", true);
            return PT_METASPACE;
        }
        if (seq && parse_split_chain(seq, m)) return PT_SPLIT_CHAIN;
        if (seq && parse_digits_bytelevel(seq, m)) return PT_DIGITS_GPT2;
        throw Unsupported("pre_tokenizer: this Sequence is outside the hot path");
    }
    throw Unsupported("pre_tokenizer: type '" + type + "' is outside the hot path");
}

}  // namespace

// hash of a long vocabulary key (tables.hpp: long_key_hash_*); the name is historical
uint32_t fnv1a(const uint8_t* p, size_t n) {
    uint32_t h = long_key_hash_init((uint32_t)n);
    for (size_t i = 0; i < n; i += 4) {
        uint32_t w = 0;
        for (size_t q = 0; q < 4 && i + q < n; ++q) w |= (uint32_t)p[i + q] << (8 * q);
        h = long_key_hash_step(h, w);
    }
    return h;
}

// str::replace of a non-empty literal: every match, left to right, none overlapping
static std::string replace_all(const std::string& t, const std::string& from, const std::string& to) {
    std::string out;
    size_t pos = 0;
    for (;;) {
        const size_t hit = t.find(from, pos);
        if (hit == std::string::npos) { out.append(t, pos, std::string::npos); break; }
        out.append(t, pos, hit - pos);
        out += to;
        pos = hit + from.size();
    }
    return out;
}

// WordPiece decoder cleanup (decoders/wordpiece.rs:31-44): eleven literal replacements applied in order
static std::string wp_cleanup(std::string t) {
    static const char* const rules[][2] = {{" .", "."}, {" ?", "?"}, {" !", "!"}, {" ,", ","}, {" ' ", "'"}, {" n't", "n't"},
                                           {" 'm", "'m"}, {" do not", " don't"}, {" 's", "'s"}, {" 've", "'ve"}, {" 're", "'re"}};
    for (auto& r : rules) t = replace_all(t, r[0], r[1]);
    return t;
}

// decode_batch tables.  Tokenizer::decode (tokenizer/mod.rs:935-953) maps every id to a token string (added
// vocabulary first, then the model; unknown ids vanish), drops specials on request and hands the strings to the
// decoder, whose result is joined.  For the decoders on this path the contribution of a token depends only on its id
// and on whether it is the first kept token of its sequence:
//   ByteLevel (pre_tokenizers/byte_level.rs:155-171)  bytes of the token through the inverse byte alphabet, or the
//                                                     token's own UTF-8 if a char is outside the alphabet
//   WordPiece (decoders/wordpiece.rs:46-64)           first: token; later: token minus the prefix, or " " + token;
//                                                     then cleanup()
//   none      (mod.rs:950-952)                        tokens.join(" ")
// so decoding is a gather of precomputed byte strings.
// by_index (Unigram): id -> piece of an array vocabulary, where two ids may share a piece and `vocab` only knows the later one
static void build_decode_tables(HostModel& m, const JsonValue* root, const std::unordered_map<std::string, uint32_t>& vocab,
                                const std::unordered_map<uint32_t, uint8_t>& c2b, const std::vector<std::string>* by_index = nullptr) {
    const JsonValue* dec = root->get("decoder");
    std::string prefix = "##", suffix = "</w>", ctc_pad, ctc_delim, post_strip;
    bool cleanup = true, chain_bytes = false;
    struct DecEl { int kind; std::string a, b; int64_t start, stop; };      // 0: Replace a -> b; 1: Strip a (one char), start / stop
    std::vector<DecEl> chain;
    auto replace_lit = [](const std::string& t, const std::string& from, const std::string& to) {
        if (!from.empty()) return replace_all(t, from, to);
        std::string out = to;                  // str::replace("", to): the empty pattern matches in front of every char and at the end
        for (size_t i = 0; i < t.size();) {
            size_t j = i + 1;
            while (j < t.size() && ((uint8_t)t[j] & 0xC0u) == 0x80u) ++j;
            out.append(t, i, j - i);
            out += to;
            i = j;
        }
        return out;
    };
    // chars of a UTF-8 string as byte ranges (Strip counts chars)
    auto char_starts = [](const std::string& t) {
        std::vector<size_t> st;
        for (size_t i = 0; i < t.size(); ++i) if (((uint8_t)t[i] & 0xC0u) != 0x80u) st.push_back(i);
        st.push_back(t.size());
        return st;
    };
    auto strip = [&](const std::string& t, const std::string& c, int64_t start, int64_t stop) {
        const std::vector<size_t> cs = char_starts(t);
        const size_t n = cs.size() - 1;
        auto is_c = [&](size_t k) { return t.compare(cs[k], cs[k + 1] - cs[k], c) == 0; };
        size_t a = 0, b = n;
        for (size_t k = 0; k < n && (int64_t)k < start; ++k) { if (!is_c(k)) break; a = k + 1; }
        for (int64_t k = 0; k < stop && (size_t)k < n; ++k) { const size_t j = n - (size_t)k - 1; if (!is_c(j)) break; b = j; }
        return b >= a ? t.substr(cs[a], cs[b] - cs[a]) : std::string();
    };
    if (!dec || dec->is_null()) m.decoder = DEC_JOIN_SPACE;
    else {
        const std::string t = dec->get_str("type");
        if (t == "ByteLevel") m.decoder = DEC_BYTELEVEL;
        else if (t == "WordPiece") {
            m.decoder = DEC_WORDPIECE;
            prefix = dec->get_str("prefix", "##");
            cleanup = dec->get_bool("cleanup", true);
        } else if (t == "BPEDecoder") {
            m.decoder = DEC_BPE;
            suffix = dec->get_str("suffix", "</w>");
            if (suffix.empty()) {        // (str::replace("", " ") puts a space between all chars: not a shape worth tables)
                m.decoder = DEC_UNSUPPORTED;
                m.dec_unsupported = "BPEDecoder with an empty suffix is outside the decode path";
                return;
            }
        } else if (t == "ByteFallback") m.decoder = DEC_BYTE_FALLBACK;
        else if (t == "Fuse") m.decoder = DEC_FUSE;
        else if (t == "CTC") {
            // decoders/ctc.rs:45-63: consecutive equal tokens collapse (on the device: an id equal to the kept id in front of it), then per
            // token: pad_token -> "", cleanup() and word_delimiter_token -> " "; a token that ends up empty contributes nothing
            m.decoder = DEC_CTC;
            m.dec_dedup = true;
            ctc_pad = dec->get_str("pad_token", "<pad>");
            ctc_delim = dec->get_str("word_delimiter_token", "|");
            cleanup = dec->get_bool("cleanup", true);
        } else if (t == "Sequence" || t == "Replace" || t == "Strip") {
            // A chain (decoders/sequence.rs:26-33: every member's decode_chain in turn; Decoder::decode joins the result with "",
            // tokenizer/mod.rs:184-187) of the per-token members -- Replace with a literal pattern (normalizers/replace.rs:88-106), Strip
            // (decoders/strip.rs:27-60) --, then ByteFallback, then Fuse, then Strip { start <= 1, stop 0 }: what the SentencePiece-style
            // tokenizers carry ([Replace("\u2581", " "), ByteFallback, Fuse, Strip(" ", 1, 0)]).  Behind Fuse there is ONE string, so that Strip
            // only ever looks at the first kept token -- its first-position form.  Anything else is refused.
            std::vector<const JsonValue*> members;
            if (t == "Sequence") {
                const JsonValue* ds = dec->get("decoders");
                if (ds && ds->is_array()) for (const auto& d : ds->arr) members.push_back(d.get());
            } else members.push_back(dec);
            int stage = 0;                      // 0: per-token members, 1: behind ByteFallback, 2: behind Fuse, 3: behind the leading Strip
            auto refuse = [&](const std::string& why) { m.decoder = DEC_UNSUPPORTED; m.dec_unsupported = why; };
            m.decoder = DEC_CHAIN;
            for (const JsonValue* d : members) {
                const std::string k = d->get_str("type");
                if (k == "Replace" && stage == 0) {
                    const JsonValue* pat = d->get("pattern");
                    const std::string lit = pat ? pat->get_str("String") : "";
                    if (lit.empty()) { refuse("a Replace decoder with a Regex (or empty) pattern is outside the decode path"); return; }
                    chain.push_back(DecEl{0, lit, d->get_str("content"), 0, 0});
                } else if (k == "Strip" && (stage == 0 || stage == 2)) {
                    const std::string c = d->get_str("content");
                    const int64_t a = (int64_t)d->get_num("start", 0), b = (int64_t)d->get_num("stop", 0);
                    if (c.empty() || a < 0 || b < 0) { refuse("a Strip decoder without a content char"); return; }
                    if (stage == 2) {
                        if (a > 1 || b != 0) { refuse("a Strip decoder behind Fuse with start > 1 or stop > 0 is outside the decode path"); return; }
                        if (a == 1) { post_strip = c; stage = 3; }
                    } else chain.push_back(DecEl{1, c, "", a, b});
                } else if (k == "ByteFallback" && stage == 0) { chain_bytes = true; stage = 1; }
                else if (k == "Fuse" && stage <= 1) stage = 2;
                else { refuse("decoder '" + k + "' at this place of a decoder Sequence is outside the decode path"); return; }
            }
            if (chain_bytes && !post_strip.empty() && (uint8_t)post_strip[0] >= 0x80u) { refuse("a non-ASCII Strip behind ByteFallback is outside the decode path"); return; }
        } else {
            m.decoder = DEC_UNSUPPORTED;
            m.dec_unsupported = "decoder type '" + t + "' is outside the decode path";
            return;
        }
    }
    // id -> token string: model vocabulary, overridden by the added vocabulary (added_vocabulary.rs:239-246)
    uint32_t n_ids = 0;
    for (auto& kv : vocab) n_ids = std::max(n_ids, kv.second + 1);
    if (by_index) n_ids = std::max(n_ids, (uint32_t)by_index->size());
    for (const AddedToken& a : m.added_tokens) n_ids = std::max(n_ids, a.id + 1);
    if (n_ids > (1u << 26)) { m.decoder = DEC_UNSUPPORTED; m.dec_unsupported = "token ids beyond 2^26"; return; }
    std::vector<const std::string*> tok(n_ids, nullptr);
    std::vector<uint8_t> special(n_ids, 0);
    for (auto& kv : vocab) tok[kv.second] = &kv.first;
    if (by_index)
        for (size_t i = 0; i < by_index->size(); ++i) tok[i] = &(*by_index)[i];
    std::unordered_map<std::string, bool> special_set;
    for (const AddedToken& a : m.added_tokens) {
        if (a.normalized && m.norm != NORM_NONE) {
            m.decoder = DEC_UNSUPPORTED;
            m.dec_unsupported = "added token '" + a.content + "' is normalized behind a normalizer (its decoded form is version dependent)";
            return;
        }
        tok[a.id] = &a.content;
        if (a.special) special_set[a.content] = true;
    }
    for (uint32_t id = 0; id < n_ids; ++id)
        if (tok[id] && special_set.count(*tok[id])) special[id] = 1;     // is_special_token tests the STRING (added_vocabulary.rs:258-260)
    m.dec_entry.assign((size_t)n_ids * 4, 0);
    m.dec_position_dependent = false;
    auto put = [&](const std::string& bytes) -> std::pair<uint32_t, uint32_t> {
        uint32_t off = (uint32_t)m.dec_blob.size();
        m.dec_blob.insert(m.dec_blob.end(), bytes.begin(), bytes.end());
        return {off, (uint32_t)bytes.size()};
    };
    for (uint32_t id = 0; id < n_ids; ++id) {
        uint32_t* e = &m.dec_entry[(size_t)id * 4];
        if (!tok[id]) { e[1] = DEC_ABSENT; continue; }
        const std::string& t = *tok[id];
        std::string first, rest;
        if (m.decoder == DEC_BYTELEVEL) {
            if (!bytelevel_to_raw(t, c2b, &first)) first = t;
            rest = first;
        } else if (m.decoder == DEC_WORDPIECE) {
            first = t;
            if (!prefix.empty() && t.compare(0, prefix.size(), prefix) == 0) rest = t.substr(prefix.size());
            else if (prefix.empty()) rest = t;                 // strip_prefix("") always succeeds
            else rest = " " + t;
            if (cleanup) { first = wp_cleanup(first); rest = wp_cleanup(rest); }
        } else if (m.decoder == DEC_BPE) {
            // token.replace(suffix, " "), and token.replace(suffix, "") on the LAST token (decoders/bpe.rs:30-37): `first` is the form of
            // the position that has one of its own -- here the last kept token (dec_special_is_last)
            first = replace_all(t, suffix, "");
            rest = replace_all(t, suffix, " ");
        } else if (m.decoder == DEC_CTC) {
            // (an empty pad_token replaces nothing by nothing; an empty word_delimiter_token puts a space in front of every char of
            // the cleaned token and one at its end, as str::replace does -- " " for a token the pad emptied)
            first = replace_lit(t, ctc_pad, "");
            if (cleanup) first = replace_lit(wp_cleanup(first), ctc_delim, " ");
            rest = first;
        } else if (m.decoder == DEC_FUSE || m.decoder == DEC_BYTE_FALLBACK || m.decoder == DEC_CHAIN) {
            std::string u = t;
            for (const DecEl& el : chain) u = el.kind == 0 ? replace_lit(u, el.a, el.b) : strip(u, el.a, el.start, el.stop);
            const std::string& t = u;                       // (what ByteFallback / Fuse see)
            first = rest = t;
            if (!post_strip.empty()) {
                // Strip(c, 1, 0) behind Fuse: one leading c off the FUSED string -- off the first kept token.  (An empty token would hand the
                // strip on to its successor: no table says that.)
                if (t.empty() && !special[id]) { m.decoder = DEC_UNSUPPORTED; m.dec_unsupported = "a token that decodes to nothing in front of a Strip behind Fuse"; return; }
                first = strip(t, post_strip, 1, 0);
            }
            const bool bytes_on = m.decoder == DEC_BYTE_FALLBACK || chain_bytes;
            // <0xXX>: six bytes, "<0x", two hex digits as u8::from_str_radix reads them (a leading '+' counts as a digit's place), ">"
            if (bytes_on && t.size() == 6 && t.compare(0, 3, "<0x") == 0 && t[5] == '>') {
                auto hex = [](char c) -> int { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
                int v = -1;
                if (t[3] == '+') { const int lo = hex(t[4]); if (lo >= 0) v = lo; }
                else { const int hi = hex(t[3]), lo = hex(t[4]); if (hi >= 0 && lo >= 0) v = hi * 16 + lo; }
                if (v >= 0) {
                    // (as the first kept token under a leading Strip of this very byte: nothing -- unless its run is not UTF-8, which the
                    // device decides: the length of the first-position form is 0 then)
                    const bool gone_first = !post_strip.empty() && post_strip.size() == 1 && (uint8_t)post_strip[0] == (uint8_t)v;
                    if (gone_first) m.dec_position_dependent = true;
                    e[0] = (uint32_t)v;
                    e[1] = (gone_first ? 0u : 1u) | DEC_BYTE | (special[id] ? DEC_SPECIAL : 0u);
                    e[2] = (uint32_t)v;
                    e[3] = 1u;
                    m.dec_has_bytes = true;
                    continue;
                }
            }
        } else {
            first = t;
            rest = " " + t;
        }
        if (first.size() > DEC_LEN_MASK || rest.size() > DEC_LEN_MASK) { m.decoder = DEC_UNSUPPORTED; m.dec_unsupported = "token too long"; return; }
        auto a = put(first);
        e[0] = a.first;
        e[1] = a.second | (special[id] ? DEC_SPECIAL : 0u);
        if (rest == first) { e[2] = a.first; e[3] = a.second; }
        else { auto b = put(rest); e[2] = b.first; e[3] = b.second; m.dec_position_dependent = true; }
    }
    m.dec_special_is_last = m.decoder == DEC_BPE;
    m.dec_blob.resize(m.dec_blob.size() + 16, 0);                        // readable slack for vector loads
}

// ==== HostModel::from_json, stage by stage (its table of contents is from_json itself, at the end).  The stages run in the order the
// sections were always read in, and THE ORDER IS PART OF THE RESULT: a file with two faults gets the message of the refusal asked first,
// and the vocabulary map is walked in the order it was filled in, which lays out every table.  tests/test_host_model_outcomes.py pins
// both: no refusal moves, merges or changes its words unless that test's golden data changes with it.
namespace {

// What the stages from read_vocab on share of the model section.  Never copied: the iteration order of `id` decides raw_tokens and
// through them the layout of every table, and a copy of an unordered_map need not iterate like its source.
struct Vocab {
    const JsonValue* model = nullptr;                // the "model" section
    std::string mtype;                               // its type, the legacy untagged spellings resolved
    bool unigram = false;
    std::unordered_map<std::string, uint32_t> id;    // piece -> id; what added tokens, templates, padding and the decode tables read
    std::vector<std::string> uni_pieces;             // Unigram: id -> piece, per index (id_to_token, unigram/model.rs:483-485)
    uint32_t b2c[256];                               // the GPT-2 byte alphabet and its inverse
    std::unordered_map<uint32_t, uint8_t> c2b;
    Vocab() {
        build_bytes_char(b2c);
        for (int b = 0; b < 256; ++b) c2b[b2c[b]] = (uint8_t)b;
    }
    Vocab(const Vocab&) = delete;
};

// ---- small things the stages share (the readers of sections stand in front of parse_pretok) ----
// the class flags of a code point (uc_stage1 / uc_stage2 must be built)
uint32_t uc_flags(const HostModel& m, uint32_t cp) { return cp < 0x110000u ? m.uc_stage2[((size_t)m.uc_stage1[cp >> 8] << 8) | (cp & 255u)] : 0u; }
bool opt_str(const JsonValue* section, const char* key, std::string* out) {
    const JsonValue* x = section->get(key);
    if (x && x->is_string()) { *out = x->str; return true; }
    return false;
}
// the id of the byte token "<0xXX>" of byte b, or null; *spelt (if given): the token
const uint32_t* byte_token_id(const Vocab& v, int b, std::string* spelt = nullptr) {
    char code[8];
    snprintf(code, sizeof(code), "<0x%02X>", b);
    if (spelt) *spelt = code;
    auto it = v.id.find(code);
    return it == v.id.end() ? nullptr : &it->second;
}
// has_unk / unk_id of a model that names its unk token
void lookup_unk(const Vocab& v, HostModel& m) {
    auto it = v.id.find(m.unk_token);
    if (it != v.id.end()) { m.has_unk = true; m.unk_id = it->second; }
}

// ---- 1. truncation / padding: an epilogue over the finished token CSR (tokenizer/mod.rs:1265-1317) ----
// reads "truncation", "padding"; writes trunc_*, pad_*.  (Its two Invalid refusals come before every other section's.)
void parse_truncation_padding(const JsonValue* root, HostModel& m) {
    const JsonValue* trunc = root->get("truncation");
    if (trunc && !trunc->is_null()) {
        m.trunc_on = true;
        m.trunc_max_length = (uint32_t)trunc->get_num("max_length", 512);
        m.trunc_stride = (uint32_t)trunc->get_num("stride", 0);
        m.trunc_left = trunc->get_str("direction", "Right") == "Left";
        const std::string st = trunc->get_str("strategy", "LongestFirst");
        if (st == "LongestFirst") m.trunc_strategy = 0;
        else if (st == "OnlyFirst") m.trunc_strategy = 1;
        else if (st == "OnlySecond") m.trunc_strategy = 2;
        else throw Invalid("tokenizer.json: unknown truncation strategy '" + st + "'");
    }
    const JsonValue* pad = root->get("padding");
    if (pad && !pad->is_null()) {
        m.pad_on = true;
        const JsonValue* ps = pad->get("strategy");
        if (ps && ps->is_object() && ps->get("Fixed")) { m.pad_fixed = true; m.pad_length = (uint32_t)ps->get_num("Fixed", 0); }
        else if (ps && ps->is_string() && ps->str == "BatchLongest") m.pad_fixed = false;
        else throw Invalid("tokenizer.json: bad padding strategy");
        m.pad_left = pad->get_str("direction", "Right") == "Left";
        const JsonValue* mult = pad->get("pad_to_multiple_of");
        m.pad_multiple = (mult && mult->is_number()) ? (uint32_t)mult->num : 0u;
        m.pad_id = (uint32_t)pad->get_num("pad_id", 0);
        m.pad_type_id = (uint32_t)pad->get_num("pad_type_id", 0);
        m.pad_token = pad->get_str("pad_token", "[PAD]");
        if (m.pad_id >= (1u << 24)) throw Unsupported("padding id beyond 2^24");
    }
}

// ---- 2. normalizer: one reader per family, picked by parse_normalizer ----
void parse_bert_normalizer(const JsonValue* norm, HostModel& m) {
    m.norm = NORM_BERT;
    m.bn_clean_text = norm->get_bool("clean_text", true);
    m.bn_handle_chinese = norm->get_bool("handle_chinese_chars", true);
    m.bn_lowercase = norm->get_bool("lowercase", true);
    const JsonValue* sa = norm->get("strip_accents");
    m.bn_strip_accents = (sa && sa->is_bool()) ? sa->b : m.bn_lowercase;  // normalizers/bert.rs:124
}

// Precompiled, alone or first in a Sequence (seq: its members) whose only other member may be the Replace(Regex " {2,}" -> " ") of XLM-R / T5
// files: behind WhitespaceSplit that member is inert (it touches runs of spaces alone, which the split drops), so no kernel runs for it --
// parse_pretok refuses it in front of anything else
void parse_precompiled(const JsonValue* norm, const JsonValue* seq, HostModel& m) {
    const JsonValue* pc = norm;
    if (seq) {
        const auto& arr = seq->arr;
        pc = arr[0].get();
        for (size_t k = 1; k < arr.size(); ++k) {
            const JsonValue* r = arr[k].get();
            const std::string rt = member_type(r);
            const JsonValue* pat = rt == "Replace" ? r->get("pattern") : nullptr;
            if (k != 1 || arr.size() != 2 || !pat || !pat->is_object() || !pat->get("Regex") || pat->get_str("Regex") != " {2,}" || r->get_str("content") != " ")
                throw Unsupported("normalizer: '" + rt + "' behind Precompiled in a Sequence is outside the hot path (only Replace(Regex ' {2,}' -> ' ') is on it)");
            m.pc_space_runs = true;
        }
    }
    const JsonValue* cm = pc->get("precompiled_charsmap");
    if (!cm || !cm->is_string()) throw Unsupported("normalizer: Precompiled without a precompiled_charsmap string");
    std::string blob;
    if (!base64_decode(cm->str, &blob)) throw Unsupported("normalizer: Precompiled precompiled_charsmap is not base64");
    m.set_precompiled(blob);
    m.norm = NORM_PRECOMPILED;
}

// A Sequence that holds NFC.  NFC alone inside a Sequence is NFC; next to any other normalizer the alignment of one is the input of the
// other: not on the path ... but for the chain of the CLIP files, Sequence[NFC, Replace(Regex "\\s+" -> " "), Lowercase]: Lowercase is a
// map of single chars that the NFC core applies to what it composed (nfc_core.hpp NFC_LOWER), and the Replace only touches runs of \s
// chars, which the CLIP pre-tokenizer drops -- it is inert there, and no kernel runs for it (but for the normalized added tokens:
// nfc_ws_fold).
// LOOKS AHEAD: the chain is accepted only if the file's pre-tokenizer is a Sequence of two that opens with a Split of the CLIP pattern --
// the one place the normalizer reads "pre_tokenizer", and it reads the pattern alone.  Whether that pre-tokenizer is the CLIP one in
// full is parse_pretok's to say; finish_pretok refuses the chain if it was not.
void parse_nfc_sequence(const JsonValue* root, const JsonValue* seq, HostModel& m) {
    const auto& arr = seq->arr;
    if (arr.size() != 1) {
        const std::string base = "normalizer: NFC inside a longer Sequence is outside the hot path (only NFC alone, or Sequence[NFC], is on it; and "
                                 "Sequence[NFC, Replace(Regex '\\s+' -> ' '), Lowercase], with or without the Replace, in front of the CLIP pre-tokenizer: ";
        auto ty = [&](size_t k) { return member_type(arr[k].get()); };
        const bool shape = (arr.size() == 2 && ty(0) == "NFC" && ty(1) == "Lowercase") || (arr.size() == 3 && ty(0) == "NFC" && ty(1) == "Replace" && ty(2) == "Lowercase");
        if (!shape) throw Unsupported(base + "this Sequence has other members, or these in another order)");
        if (arr.size() == 3) {
            const JsonValue* pat = arr[1]->get("pattern");
            if (!pat || !pat->is_object() || !pat->get("Regex") || pat->get_str("Regex") != "\\s+" || arr[1]->get_str("content") != " ")
                throw Unsupported(base + "this Sequence's Replace is another one)");
            m.nfc_ws_fold = true;
        }
        const JsonValue* pt = root->get("pre_tokenizer");
        const JsonValue* pts = member_type(pt) == "Sequence" ? members_of(pt, "pretokenizers") : nullptr;
        const JsonValue* sp = (pts && pts->arr.size() == 2 && member_type(pts->arr[0].get()) == "Split") ? pts->arr[0]->get("pattern") : nullptr;
        if (!sp || !sp->is_object() || sp->get_str("Regex") != kClipPattern) throw Unsupported(base + "this file's pre-tokenizer is another one)");
        m.nfc_lower = true;
    }
    m.norm = NORM_NFC;
}

// NFD, Lowercase, StripAccents: alone (t), or a Sequence of them (seq).  What the file says is read here; whether it is on the path in
// front of this file's pre-tokenizer and model is decided by check_normalizer_against_pretok_type and check_layout, once they are
// known, in the words this section was refused by
void parse_norm_chain(const std::string& t, const JsonValue* seq, HostModel& m) {
    m.chain_spelling = t == "Sequence" ? "this Sequence" : "type '" + t + "'";
    if (t == "Sequence") {
        for (const JsonPtr& v : seq->arr) {
            const std::string mt = member_type(v.get());
            const int k = chain_member(mt);
            if (k < 0) throw Unsupported("normalizer: '" + mt + "' next to NFD / Lowercase / StripAccents in a Sequence is outside the hot path (only these three chain)");
            if (m.chain_has((uint8_t)k)) throw Unsupported("normalizer: '" + mt + "' twice in a Sequence is outside the hot path");
            if (k == CHAIN_NFD && m.chain_has(CHAIN_STRIP_ACCENTS))
                throw Unsupported("normalizer: 'StripAccents' in front of 'NFD' in a Sequence is outside the hot path (the marks NFD splits off afterwards stay, "
                                  "in the order the text around them decides)");
            m.chain.push_back((uint8_t)k);
        }
    } else m.chain.push_back((uint8_t)chain_member(t));
    m.norm = NORM_CHAIN;
}

// NFKC alone, or alone inside a Sequence (seq, else null).  What the file says is read here; a Sequence with more in it is only NOTED
// (nfkc_refusal): check_normalizer_against_pretok_type throws it once the pre-tokenizer's type is known, behind the words the type
// was always refused by
void parse_nfkc(const JsonValue* seq, HostModel& m) {
    if (seq) {
        for (const JsonPtr& v : seq->arr) {
            const std::string mt = member_type(v.get());
            if (mt == "NFKC") continue;
            m.nfkc_refusal = "normalizer: '" + mt + "' next to NFKC in a Sequence is outside the hot path (only NFKC alone, or Sequence[NFKC], is on it)";
            break;
        }
        if (m.nfkc_refusal.empty() && seq->arr.size() != 1)
            m.nfkc_refusal = "normalizer: 'NFKC' twice in a Sequence is outside the hot path (only NFKC alone, or Sequence[NFKC], is on it)";
    }
    m.norm = NORM_NFKC;
}

// the "▁" normalizers of SentencePiece conversions: Sequence[Prepend("▁"), Replace(" " -> "▁")] (Llama-2, Mistral) or
// Replace(" " -> "▁") alone (Gemma-style); anything else of these types is outside the path
void parse_u2581_normalizers(const JsonValue* norm, const std::string& t, HostModel& m) {
    auto is_replace = [](const JsonValue* r) {
        if (!r || r->get_str("type") != "Replace") return false;
        const JsonValue* pat = r->get("pattern");
        if (!pat || !pat->is_object() || !pat->get("String")) throw Unsupported("normalizer: Replace with a Regex pattern");
        if (pat->get_str("String") != " ") throw Unsupported("normalizer: Replace of '" + pat->get_str("String") + "' (only ' ' -> U+2581 is on the path)");
        if (r->get_str("content") != kMetaspace) throw Unsupported("normalizer: Replace with '" + r->get_str("content") + "' (only ' ' -> U+2581 is on the path)");
        return true;
    };
    auto is_prepend = [](const JsonValue* r) {
        if (!r || r->get_str("type") != "Prepend") return false;
        if (r->get_str("prepend") != kMetaspace) throw Unsupported("normalizer: Prepend of '" + r->get_str("prepend") + "' (only U+2581 is on the path)");
        return true;
    };
    const JsonValue* seq = t == "Sequence" ? members_of(norm, "normalizers") : nullptr;
    if (t == "Replace" && is_replace(norm)) m.ms_prepend = MS_NEVER;
    else if (seq && seq->arr.size() == 2 && is_prepend(seq->arr[0].get()) && is_replace(seq->arr[1].get())) m.ms_prepend = MS_PIECE;
    else throw Unsupported("normalizer: this " + t + " is outside the hot path (only Sequence[Prepend(U+2581), Replace(' ' -> U+2581)] and "
                           "Replace(' ' -> U+2581) are)");
    m.norm = NORM_METASPACE;
}

// reads "normalizer" (and, for the CLIP chain alone, the Split pattern of "pre_tokenizer": parse_nfc_sequence); writes norm and the
// family's options (bn_*, pc_*, chain, chain_spelling, nfkc_refusal, nfc_lower, nfc_ws_fold, ms_prepend).  The families are asked in this
// order: a Sequence that holds members of two of them belongs to the first.
void parse_normalizer(const JsonValue* root, HostModel& m) {
    const JsonValue* norm = root->get("normalizer");
    if (!norm || norm->is_null()) return;
    const std::string t = norm->get_str("type");
    const JsonValue* seq = t == "Sequence" ? members_of(norm, "normalizers") : nullptr;
    auto holds = [&](auto&& is_one) { return seq && std::any_of(seq->arr.begin(), seq->arr.end(), [&](const JsonPtr& v) { return is_one(member_type(v.get())); }); };
    if (t == "BertNormalizer") parse_bert_normalizer(norm, m);
    else if (t == "NFC") m.norm = NORM_NFC;
    else if (t == "Precompiled" || (seq && !seq->arr.empty() && member_type(seq->arr[0].get()) == "Precompiled")) parse_precompiled(norm, seq, m);
    else if (seq && seq->arr.empty()) {
        // Sequence[] applies nothing (normalizers/utils.rs: a loop over no normalizer): DeepSeek-V3 files carry it
    } else if (holds([](const std::string& ty) { return ty == "NFC"; })) parse_nfc_sequence(root, seq, m);
    else if (chain_member(t) >= 0 || holds([](const std::string& ty) { return chain_member(ty) >= 0; })) parse_norm_chain(t, seq, m);
    else if (t == "NFKC" || holds([](const std::string& ty) { return ty == "NFKC"; })) parse_nfkc(seq, m);
    else if (t == "Sequence" || t == "Replace" || t == "Prepend") parse_u2581_normalizers(norm, t, m);
    else throw Unsupported("normalizer: type '" + t + "' is outside the hot path");
}

// ---- 3. the normalizer against the pre-tokenizer's TYPE ----
// LOOKS AHEAD: reads the type (and Metaspace's split) of "pre_tokenizer" before parse_pretok does, so that a chain or an NFKC in front of
// the wrong pre-tokenizer is refused as the NORMALIZER it is, in front of parse_pretok's own refusals of a normalizer ("Metaspace behind
// a normalizer", ...).  reads norm, chain_spelling, nfkc_refusal; writes nothing.
void check_normalizer_against_pretok_type(const JsonValue* root, const HostModel& m) {
    const JsonValue* pt = root->get("pre_tokenizer");
    const std::string ptype = type_name_or_null(pt);
    if (m.norm == NORM_CHAIN) {
        if (ptype != "Whitespace" && ptype != "WhitespaceSplit" && ptype != "BertPreTokenizer") throw Unsupported(chain_refusal(m, "pre_tokenizer '" + ptype + "'"));
    }
    if (m.norm == NORM_NFKC) {
        if (ptype != "Metaspace") throw Unsupported("normalizer: type 'NFKC' is outside the hot path");
        if (!m.nfkc_refusal.empty()) throw Unsupported(m.nfkc_refusal);
        if (!pt->get_bool("split", true))
            throw Unsupported("pre_tokenizer: Metaspace(split = false) behind NFKC is outside the hot path (only split = true is on it behind the normalizer)");
    }
}

// ---- 5. what follows from the pre-tokenizer's kind (4. is parse_pretok, above) ----
// reads pretok, split_rule, norm, nfc_lower; writes the second class table ucc_stage1 / 2.  Its three refusals stand behind all of
// parse_pretok's and in front of the post-processor's and the model's.
void finish_pretok(HostModel& m) {
    // the case classes of the case-split letter alternatives
    if (m.pretok == PT_LLAMA3 && m.split_rule.letters == 2) two_stage(flat_of(kUcCaseRuns), &m.ucc_stage1, &m.ucc_stage2);
    if (m.pretok == PT_SPLIT_CHAIN) {                                  // \p{P}, \p{S}, \p{M} for the chain's third pattern: the same slot, the rule's second class table
        if (m.norm != NORM_NONE && m.norm != NORM_NFC)
            throw Unsupported("pre_tokenizer: the chained Split behind a normalizer other than NFC");
        two_stage(flat_of(kUcPsmRuns), &m.ucc_stage1, &m.ucc_stage2);
    }
    if (m.pretok == PT_DIGITS_GPT2 && m.norm != NORM_NONE && m.norm != NORM_NFC)
        throw Unsupported("pre_tokenizer: Sequence[Digits, ByteLevel] behind a normalizer other than NFC");
    // (parse_nfc_sequence looked at the Split's pattern alone; everything else of the CLIP pre-tokenizer was parse_pretok's to accept)
    if (m.nfc_lower && m.pretok != PT_CLIP)
        throw Unsupported("normalizer: NFC inside a longer Sequence is outside the hot path (only NFC alone, or Sequence[NFC], is on it; and "
                          "Sequence[NFC, Replace(Regex '\\s+' -> ' '), Lowercase] in front of the CLIP pre-tokenizer, which this file's is not)");
}

// ---- 6. post-processor: offset trimming + the special tokens it puts around a single sequence and a pair ----
// the ids a template's SpecialToken piece stands for
const JsonValue* template_special_ids(const JsonValue* special_tokens, const std::string& name) {
    const JsonValue* def = special_tokens ? special_tokens->get(name.c_str()) : nullptr;
    const JsonValue* ids = def ? def->get("ids") : nullptr;
    if (!ids || !ids->is_array()) throw Invalid("tokenizer.json: TemplateProcessing special token '" + name + "' is not defined");
    return ids;
}

// [cls] A [sep]   (processors/bert.rs:51-120, roberta.rs); t: which of the two the untagged enum makes of the section
void apply_bert_roberta(const JsonValue* pp, const std::string& t, HostModel& m) {
    const JsonValue* cls = pp->get("cls");
    const JsonValue* sep = pp->get("sep");
    if (!cls || !sep || !cls->is_array() || !sep->is_array() || cls->arr.size() != 2 || sep->arr.size() != 2)
        throw Invalid("tokenizer.json: bad cls/sep in post_processor");
    m.pp_prefix.insert(m.pp_prefix.begin(), (uint32_t)cls->arr[1]->num);
    m.pp_suffix.push_back((uint32_t)sep->arr[1]->num);
    m.pp_prefix_ty.insert(m.pp_prefix_ty.begin(), (uint8_t)0);
    m.pp_suffix_ty.push_back((uint8_t)0);
    if (m.pp_single_typed) m.pp_unsupported = "a TemplateProcessing with type ids combined with another post-processor";
    if (!m.pp_pair.empty()) m.pp_pair_unsupported = "two post-processors that add special tokens";
    const uint32_t c = (uint32_t)cls->arr[1]->num, e = (uint32_t)sep->arr[1]->num;
    if (t == "BertProcessing")         // [CLS] A [SEP] : 0   B [SEP] : 1          (processors/bert.rs:121-150)
        m.pp_pair = {{2, c, 0}, {0, 0, 0}, {2, e, 0}, {1, 0, 1}, {2, e, 1}};
    else                               // <s> A </s> </s> B </s>, all type 0        (processors/roberta.rs)
        m.pp_roberta = true, m.pp_pair_plain = {{0, 0, 0}, {1, 0, 0}}, m.pp_pair = {{2, c, 0}, {0, 0, 0}, {2, e, 0}, {2, e, 0}, {1, 0, 0}, {2, e, 0}};
}

// TemplateProcessing's `single` template (processors/template.rs:544-590).  One that is not "ids around sequence A" is refused when a
// single sequence is encoded with special tokens (pp_unsupported) -- the pair template is parsed regardless
void apply_template_single(const JsonValue* pp, const JsonValue* sp, HostModel& m) {
    const JsonValue* single = pp->get("single");
    if (!single || !single->is_array()) throw Invalid("tokenizer.json: TemplateProcessing without `single`");
    std::vector<uint32_t> pre, post;
    std::vector<uint8_t> pre_ty, post_ty;
    double seq_ty = 0, max_ty = 0;
    int n_seq = 0;
    for (auto& piece : single->arr) {
        if (const JsonValue* sq = piece->get("Sequence")) {
            if (sq->get_str("id") != "A") m.pp_unsupported = "TemplateProcessing single template refers to sequence B";
            seq_ty = sq->get_num("type_id", 0);
            max_ty = std::max(max_ty, seq_ty);
            ++n_seq;
        } else if (const JsonValue* st = piece->get("SpecialToken")) {
            const JsonValue* ids = template_special_ids(sp, st->get_str("id"));
            const double ty = st->get_num("type_id", 0);
            max_ty = std::max(max_ty, ty);
            for (auto& x : ids->arr) { (n_seq ? post : pre).push_back((uint32_t)x->num); (n_seq ? post_ty : pre_ty).push_back((uint8_t)ty); }
        } else throw Invalid("tokenizer.json: bad TemplateProcessing piece");
    }
    if (n_seq != 1 && m.pp_unsupported.empty()) m.pp_unsupported = "TemplateProcessing single template must contain sequence A exactly once";
    if (max_ty > 255 && m.pp_unsupported.empty()) m.pp_unsupported = "TemplateProcessing type id above 255";
    if (max_ty > 0 && m.pp_unsupported.empty()) {
        // (a second post-processor would see -- and a second template overwrite -- these type ids)
        if (!m.pp_prefix.empty() || !m.pp_suffix.empty() || m.pp_single_typed) m.pp_unsupported = "a TemplateProcessing with type ids combined with another post-processor";
        else m.pp_single_typed = true, m.pp_seq_ty = (uint32_t)seq_ty;
    } else if (m.pp_single_typed && m.pp_unsupported.empty()) {
        m.pp_unsupported = "a TemplateProcessing with type ids combined with another post-processor";
    }
    if (m.pp_unsupported.empty()) {
        m.pp_prefix.insert(m.pp_prefix.begin(), pre.begin(), pre.end());
        m.pp_suffix.insert(m.pp_suffix.end(), post.begin(), post.end());
        m.pp_prefix_ty.insert(m.pp_prefix_ty.begin(), pre_ty.begin(), pre_ty.end());
        m.pp_suffix_ty.insert(m.pp_suffix_ty.end(), post_ty.begin(), post_ty.end());
    } else {
        m.pp_single_typed = false;
        m.pp_single_refused = true;           // (sequence A twice, or typed, comes out that way without special tokens too)
    }
}

// the `pair` template (processors/template.rs:544-590): any order of A, B and special tokens, each with its type id
void apply_template_pair(const JsonValue* pp, const JsonValue* sp, HostModel& m) {
    if (!m.pp_pair.empty()) m.pp_pair_unsupported = "two post-processors that add special tokens";
    const JsonValue* pair = pp->get("pair");
    if (!pair || !pair->is_array()) { m.pp_pair_unsupported = "TemplateProcessing without a `pair` template"; return; }
    int na = 0, nb = 0;
    for (auto& piece : pair->arr) {
        if (const JsonValue* sq = piece->get("Sequence")) {
            const bool is_a = sq->get_str("id") == "A";
            (is_a ? na : nb)++;
            m.pp_pair.push_back({is_a ? 0u : 1u, 0u, (uint32_t)sq->get_num("type_id", 0)});
        } else if (const JsonValue* st = piece->get("SpecialToken")) {
            const JsonValue* ids = template_special_ids(sp, st->get_str("id"));
            for (auto& x : ids->arr) m.pp_pair.push_back({2u, (uint32_t)x->num, (uint32_t)st->get_num("type_id", 0)});
        } else throw Invalid("tokenizer.json: bad TemplateProcessing piece");
    }
    if (na != 1 || nb != 1) m.pp_pair_unsupported = "TemplateProcessing pair template must contain A and B exactly once each";
    m.pp_pair_plain.clear();
    for (const HostModel::TplPiece& q : m.pp_pair)
        if (q.kind != 2u) m.pp_pair_plain.push_back(q);
    if (m.pp_pair.size() > 64) m.pp_pair_unsupported = "TemplateProcessing pair template with more than 64 pieces";
}

// one post-processor section; a Sequence applies its members in order (processors/sequence.rs)
void apply_post_processor(const JsonValue* pp, HostModel& m) {
    if (!pp || pp->is_null()) return;
    std::string t = pp->get_str("type");
    if (t == "BertProcessing" || t == "RobertaProcessing") {
        // PostProcessorWrapper is an untagged enum that tries Roberta before Bert and "serde does not validate tags"
        // (processors/mod.rs:19-23): with both of Roberta's flags present it is a RobertaProcessing whatever `type` says, else Bert
        const JsonValue* a = pp->get("trim_offsets");
        const JsonValue* b = pp->get("add_prefix_space");
        t = (a && a->is_bool() && b && b->is_bool()) ? "RobertaProcessing" : "BertProcessing";
    }
    if (t == "ByteLevel" || t == "RobertaProcessing") {
        m.trim_offsets = pp->get_bool("trim_offsets", true);
        m.pp_add_prefix_space = pp->get_bool("add_prefix_space", true);
    }
    if (t == "ByteLevel") return;
    if (t == "BertProcessing" || t == "RobertaProcessing") return apply_bert_roberta(pp, t, m);
    if (t == "TemplateProcessing") {
        const JsonValue* sp = pp->get("special_tokens");
        apply_template_single(pp, sp, m);
        apply_template_pair(pp, sp, m);
        return;
    }
    if (t == "Sequence") {
        if (const JsonValue* ps = members_of(pp, "processors"))
            for (auto& q : ps->arr) apply_post_processor(q.get(), m);
        return;
    }
    m.pp_unsupported = "post_processor type '" + t + "' is outside the hot path";
}

// reads "post_processor"; writes trim_offsets, pp_*.  Most of what it cannot take is NOTED (pp_unsupported, pp_pair_unsupported) and
// refused by the encode call that needs it; read_vocab's trim-offsets check relies on trim_offsets being known here.
void parse_post_processor(const JsonValue* root, HostModel& m) {
    apply_post_processor(root->get("post_processor"), m);
    for (size_t k = 0; k < m.pp_prefix.size(); ++k) m.pp_single.push_back({2u, m.pp_prefix[k], k < m.pp_prefix_ty.size() ? (uint32_t)m.pp_prefix_ty[k] : 0u});
    m.pp_single.push_back({0u, 0u, m.pp_single_typed ? m.pp_seq_ty : 0u});
    for (size_t k = 0; k < m.pp_suffix.size(); ++k) m.pp_single.push_back({2u, m.pp_suffix[k], k < m.pp_suffix_ty.size() ? (uint32_t)m.pp_suffix_ty[k] : 0u});
    m.pp_single_plain = {{0u, 0u, m.pp_single_typed ? m.pp_seq_ty : 0u}};
}

// ---- 7. added tokens ----
// reads "added_tokens"; writes added_tokens as the file has them (assign_added_token_ids gives them the reference's ids)
void parse_added_tokens(const JsonValue* root, HostModel& m) {
    const JsonValue* at = root->get("added_tokens");
    if (!at || !at->is_array()) return;
    for (auto& e : at->arr) {
        AddedToken a;
        a.content = e->get_str("content");
        a.id = (uint32_t)e->get_num("id", 0);
        if (e->get_num("id", 0) < 0 || a.id >= (1u << 24)) throw Unsupported("added token id beyond 2^24");
        a.special = e->get_bool("special", false);
        a.single_word = e->get_bool("single_word", false);
        a.lstrip = e->get_bool("lstrip", false);
        a.rstrip = e->get_bool("rstrip", false);
        a.normalized = e->get_bool("normalized", false);
        m.added_tokens.push_back(std::move(a));
    }
}

// ---- 8. the model's type and vocabulary ----
// a trimming post-processor (ByteLevel / RobertaProcessing) on a model that is not byte-level: process_offsets moves the offsets of every
// token whose STRING starts or ends with whitespace or 'Ġ' (byte_level.rs:202-234).  The added tokens' raw slices can (k_token_meta
// trims those); a vocabulary entry that could is outside the path
void check_trim_offsets_vocab(const Vocab& v, HostModel& m) {
    if (m.uc_stage1.empty()) build_unicode(m);
    for (auto& kv : v.id) {
        const uint8_t* b = (const uint8_t*)kv.first.data();
        const size_t n = kv.first.size();
        if (!n) continue;
        uint32_t c0 = 0, c1 = 0;
        utf8_decode(b, n, &c0);
        size_t q = n - 1;
        while (q > 0 && (b[q] & 0xC0u) == 0x80u) --q;
        utf8_decode(b + q, n - q, &c1);
        auto trimmed = [&](uint32_t c) { return c == 0x120u || (uc_flags(m, c) & UC_RUST_WS); };
        if (trimmed(c0) || trimmed(c1)) throw Unsupported("post_processor with trim_offsets on a vocabulary that is not byte-level and holds an entry with leading / trailing whitespace or 'Ġ' ('" + kv.first + "')");
    }
}

// reads "model" (type, vocab), pretok, trim_offsets, byte_level; writes v (model, mtype, unigram, id, uni_pieces), vocab_size, uni_score,
// uni_unk_score.  The pre-tokenizers that go with one model type alone refuse every other type HERE, in front of the vocabulary's own
// refusals and long before the model's parser could say "outside the hot path" of a type it does not know.
void read_vocab(const JsonValue* root, HostModel& m, Vocab& v) {
    const JsonValue* model = v.model = root->get("model");
    if (!model || !model->is_object()) throw Invalid("tokenizer.json: missing model");
    std::string& mtype = v.mtype = model->get_str("type");
    const JsonValue* vocab = model->get("vocab");
    if (mtype.empty()) {
        // legacy untagged models (models/mod.rs:71-136): BPE has merges, WordPiece has a prefix
        if (model->get("merges")) mtype = "BPE";
        else if (model->get("continuing_subword_prefix")) mtype = "WordPiece";
        else mtype = "WordLevel";
    }
    // Unigram keeps its vocabulary as an ARRAY of [piece, score], id = index (models/unigram/serialization.rs:13-30); every other model
    // as an object piece -> id.  Both fill the same map v.id
    const bool unigram = v.unigram = mtype == "Unigram";
    if (m.pretok == PT_CLIP && mtype != "BPE")
        throw Unsupported("pre_tokenizer: the CLIP Split + ByteLevel in front of a " + mtype + " model (only in front of byte-level BPE with an end_of_word_suffix is it on the path)");
    if (m.pretok == PT_BLOOM && mtype != "BPE")
        throw Unsupported("pre_tokenizer: BLOOM's Split + ByteLevel in front of a " + mtype + " model (only in front of byte-level BPE is it on the path)");
    if (m.pretok == PT_DIGITS_GPT2 && mtype != "BPE")
        throw Unsupported("pre_tokenizer: Sequence[Digits, ByteLevel] in front of a " + mtype + " model (only in front of byte-level BPE is it on the path)");
    if (unigram ? !(vocab && vocab->is_array()) : !(vocab && vocab->is_object())) throw Invalid("tokenizer.json: model.vocab missing");

    if (unigram) {
        // Unigram::from (unigram/model.rs:104-151): token_to_ids.insert in index order -- of two equal pieces the LATER id encodes --,
        // min_score over every entry (the shadowed and the unk piece included); scores are f64 as the reference's own JSON reader rounds them
        // (serde_json_f64 above: not always strtod's value)
        const size_t n = vocab->arr.size();
        if (n == 0) throw Unsupported("model: Unigram with an empty vocab (EmptyVocabulary) is outside the hot path");
        if (n >= ((size_t)1 << 24)) throw Unsupported("token id beyond 2^24 (Unigram vocab of " + std::to_string(n) + " pieces)");
        v.id.reserve(n * 2);
        v.uni_pieces.reserve(n);
        m.uni_score.reserve(n);
        double min_score = std::numeric_limits<double>::infinity();
        for (size_t i = 0; i < n; ++i) {
            const JsonValue* e = vocab->arr[i].get();
            if (!e->is_array() || e->arr.size() != 2 || !e->arr[0]->is_string() || !e->arr[1]->is_number())
                throw Invalid("tokenizer.json: Unigram vocab entry " + std::to_string(i) + " is not [piece, score]");
            v.id[e->arr[0]->str] = (uint32_t)i;
            v.uni_pieces.push_back(e->arr[0]->str);
            const double score = serde_json_f64(e->arr[1]->str);
            m.uni_score.push_back(score);
            if (score < min_score) min_score = score;
        }
        m.uni_unk_score = min_score - 10.0;      // K_UNK_PENALTY, unigram/model.rs:277
    } else {
        v.id.reserve(vocab->obj.size() * 2);
        for (auto& kv : vocab->obj) {
            if (!kv.second->is_number()) throw Invalid("tokenizer.json: vocab id is not a number");
            v.id[kv.first] = (uint32_t)kv.second->num;   // duplicate keys: last wins, like serde's map
            // the pair hashes (tables.hpp) multiply 24-bit operands and the result rows keep ids in 24 bits: larger ids would
            // collide for every seed, so they are refused here with the reason instead of failing table construction
            if (kv.second->num < 0 || kv.second->num >= (double)(1u << 24)) throw Unsupported("token id beyond 2^24 (vocab entry '" + kv.first + "')");
        }
    }
    m.vocab_size = unigram ? (uint32_t)v.uni_pieces.size() : (uint32_t)v.id.size();      // (get_vocab_size: the array's length, duplicates and all, unigram/model.rs:439-441)
    if (m.trim_offsets && !m.byte_level) check_trim_offsets_vocab(v, m);
}

// ---- 9. the ids of the added tokens ----
// The ids the reference gives the added tokens are not the ones in the file: deserialisation hands them, in file order, to
// AddedVocabulary::add_tokens (serialization.rs:153-167 -- it only WARNS when the outcome differs from the file), which gives a
// token whose content the model knows the model's id and every other one the next free id from the model's vocabulary size on; a
// content seen twice keeps its first id and its last properties (added_vocabulary.rs:272-360).  Files the library wrote agree with
// that already.
// reads v.id, vocab_size; rewrites added_tokens (build_decode_tables and build_added_patterns read the result)
void assign_added_token_ids(const Vocab& v, HostModel& m) {
    std::unordered_map<std::string, size_t> seen;
    std::vector<AddedToken> kept;
    uint32_t next_id = m.vocab_size;
    for (AddedToken& a : m.added_tokens) {
        if (a.content.empty()) continue;
        auto it = seen.find(a.content);
        if (it != seen.end()) {
            AddedToken& old = kept[it->second];
            a.id = old.id;
            old = a;
            continue;
        }
        auto vit = v.id.find(a.content);
        a.id = vit != v.id.end() ? vit->second : next_id++;
        if (a.id >= (1u << 24)) throw Unsupported("added token id beyond 2^24");
        seen[a.content] = kept.size();
        kept.push_back(a);
    }
    m.added_tokens = std::move(kept);
}

// ---- 10. the raw-byte view of the vocabulary ----
// reads v.id IN ITS ITERATION ORDER, byte_level; writes raw_tokens / raw_ids -- the order every table below is laid out in
void build_raw_tokens(const Vocab& v, HostModel& m) {
    m.raw_tokens.reserve(v.id.size());
    m.raw_ids.reserve(v.id.size());
    for (auto& kv : v.id) {
        if (m.byte_level) {
            std::string raw;
            if (!bytelevel_to_raw(kv.first, v.c2b, &raw)) continue;   // not producible from bytes
            m.raw_tokens.push_back(std::move(raw));
        } else {
            m.raw_tokens.push_back(kv.first);
        }
        m.raw_ids.push_back(kv.second);
    }
}

// ---- 12. the model's options (11. is build_decode_tables, above) ----
// BPE over characters (BPE::merge_word, bpe/model.rs:465-550): a char's initial symbol is the vocabulary entry of the char with the
// affixes its place in the word glues on.  Every (char, affix combination) the vocabulary knows goes into one direct indexed table;
// with byte_fallback, byte_id[] holds the <0xXX> tokens
void build_char_ids(const Vocab& v, HostModel& m) {
    if (m.bpe_prefix.size() > 31 || m.bpe_suffix.size() > 31) throw Unsupported("BPE continuing_subword_prefix / end_of_word_suffix longer than 31 bytes");
    m.char_id.assign(CHAR_TABLE_WORDS, CHAR_NONE);
    for (auto& kv : v.id) {
        const std::string& e = kv.first;
        for (uint32_t var = 0; var < 4; ++var) {
            if ((var & 1u) && m.bpe_prefix.empty()) continue;
            if ((var & 2u) && m.bpe_suffix.empty()) continue;
            size_t a = 0, b = e.size();
            if (var & 1u) { if (e.compare(0, m.bpe_prefix.size(), m.bpe_prefix) != 0 || e.size() < m.bpe_prefix.size()) continue; a = m.bpe_prefix.size(); }
            if (var & 2u) { if (b - a < m.bpe_suffix.size() || e.compare(b - m.bpe_suffix.size(), m.bpe_suffix.size(), m.bpe_suffix) != 0) continue; b -= m.bpe_suffix.size(); }
            if (b <= a || b - a > 4) continue;
            uint32_t cp = 0;
            const size_t l = utf8_decode((const uint8_t*)e.data() + a, b - a, &cp);
            if (l != b - a || cp >= 0x110000u) continue;                  // exactly one char between the affixes
            m.char_id[((size_t)cp << 2) | var] = kv.second;
        }
    }
    for (int b = 0; b < 256; ++b) m.byte_id[b] = CHAR_NONE;
    if (m.byte_fallback) {
        // (merge_word glues the affixes on BEFORE it falls back to bytes, so they would be spelt out as <0xXX> tokens too --
        // symbols the word has no bytes for; and a byte without its token sends the char on to the unk path behind symbols
        // already added: both corners are refused)
        if (!m.bpe_prefix.empty() || !m.bpe_suffix.empty()) throw Unsupported("BPE byte_fallback together with continuing_subword_prefix / end_of_word_suffix");
        for (int b = 0; b < 256; ++b) {
            std::string code;
            const uint32_t* id = byte_token_id(v, b, &code);
            if (!id) throw Unsupported("BPE byte_fallback without the byte token " + code);
            m.byte_id[b] = *id;
        }
    }
}

// byte-level BPE: byte -> initial symbol id (bpe/model.rs:494-499 with the byte-level alphabet), and with an end_of_word_suffix the id of
// (the byte's char + the suffix)
void build_byte_ids(const Vocab& v, HostModel& m) {
    for (int b = 0; b < 256; ++b) {
        uint8_t u[4];
        const std::string ch((const char*)u, nfc_utf8_put(u, v.b2c[b]));
        auto it = v.id.find(ch);
        if (it == v.id.end())
            throw Unsupported("byte-level BPE vocab lacks a byte symbol (unk / byte_fallback / dropped-char paths, bpe/model.rs:501-541)" +
                              (m.byte_suffix ? ": '" + ch + "'" : std::string()));
        m.byte_id[b] = it->second;
        // (with all 256 chars and all 256 char + suffix entries no word ever needs the unk_token)
        if (m.byte_suffix) {
            it = v.id.find(ch + m.bpe_suffix);
            if (it == v.id.end()) throw Unsupported("byte-level BPE with end_of_word_suffix: the vocab lacks '" + ch + m.bpe_suffix + "' (a byte's char with the suffix)");
            m.byte_sfx_id[b] = it->second;
        }
    }
}

// merges (bpe/model.rs:252-275): rank = position, new_id = vocab[a+b]; duplicate pairs: last wins.  Writes n_merges and the merge table
void parse_merges(const Vocab& v, HostModel& m) {
    const JsonValue* mg = v.model->get("merges");
    if (!mg || !mg->is_array()) throw Invalid("tokenizer.json: BPE merges missing");
    std::unordered_map<uint64_t, std::pair<uint32_t, uint32_t>> mm;
    mm.reserve(mg->arr.size() * 2);
    uint32_t rank = 0;
    for (auto& e : mg->arr) {
        std::string a, b;
        if (e->is_array() && e->arr.size() == 2 && e->arr[0]->is_string() && e->arr[1]->is_string()) {
            a = e->arr[0]->str; b = e->arr[1]->str;
        } else if (e->is_string()) {     // legacy "a b" (bpe/serialization.rs:141-149)
            size_t sp = e->str.find(' ');
            if (sp == std::string::npos || e->str.find(' ', sp + 1) != std::string::npos)
                throw Invalid("tokenizer.json: bad legacy merge entry");
            a = e->str.substr(0, sp); b = e->str.substr(sp + 1);
        } else throw Invalid("tokenizer.json: bad merge entry");
        // (new token = a + b minus the continuing_subword_prefix's LENGTH in bytes, whatever b starts with: BpeBuilder::build :246-271)
        if (b.size() < m.bpe_prefix.size()) throw Invalid("tokenizer.json: a merge's right-hand token is shorter than continuing_subword_prefix");
        auto ia = v.id.find(a), ib = v.id.find(b), in = v.id.find(a + b.substr(m.bpe_prefix.size()));
        if (ia == v.id.end() || ib == v.id.end() || in == v.id.end())
            throw Invalid("tokenizer.json: merge token out of vocabulary (MergeTokenOutOfVocabulary)");
        // the "▁" front's unit split (PT_METASPACE without split): exact only if no merge joins a char other than "▁" to a symbol that
        // starts with "▁" -- then no pair across a cut ever merges, and every unit runs its merges on its own (bpe/word.rs:162-250)
        if (m.pretok == PT_METASPACE && !m.ms_split && m.char_bpe && b.compare(0, 3, kMetaspace) == 0 && !(a.size() >= 3 && a.compare(a.size() - 3, 3, kMetaspace) == 0))
            throw Unsupported("pre_tokenizer: the merge ('" + a + "', '" + b + "') joins a char other than U+2581 to a U+2581: whole-piece BPE "
                              "(no split at U+2581) is outside the hot path for this vocabulary");
        mm[((uint64_t)ia->second << 32) | ib->second] = {rank, in->second};
        ++rank;
    }
    if (rank >= (1u << 20)) throw Unsupported("more than 2^20 merges");
    m.n_merges = rank;
    std::vector<MergeSlot> merges;
    merges.reserve(mm.size());
    for (auto& kv : mm) merges.push_back(MergeSlot{(uint32_t)(kv.first >> 32), (uint32_t)kv.first, kv.second.first, kv.second.second});
    std::sort(merges.begin(), merges.end(), [](const MergeSlot& x, const MergeSlot& y) { return x.rank < y.rank; });
    build_merge_table(m, merges);
}

// reads the BPE options, byte_level, pretok; writes model, the bpe_* / unk options, char_bpe, byte_suffix, char_id, byte_id, byte_sfx_id,
// the merge table.  check_layout's questions about char_bpe and the affixes rely on these refusals having been made first.
void parse_bpe(const Vocab& v, HostModel& m) {
    const JsonValue* model = v.model;
    m.model = MODEL_BPE;
    const JsonValue* dr = model->get("dropout");
    if (dr && dr->is_number() && dr->num != 0.0) throw Unsupported("BPE dropout needs the reference's RNG (bpe/word.rs:181)");
    opt_str(model, "continuing_subword_prefix", &m.bpe_prefix);
    opt_str(model, "end_of_word_suffix", &m.bpe_suffix);
    m.fuse_unk = model->get_bool("fuse_unk", false);
    m.byte_fallback = model->get_bool("byte_fallback", false);
    m.ignore_merges = model->get_bool("ignore_merges", false);
    if (opt_str(model, "unk_token", &m.unk_token)) {
        m.unk_configured = true;
        lookup_unk(v, m);
    }
    m.char_bpe = !m.byte_level;
    if (m.byte_level && (!m.bpe_prefix.empty() || !m.bpe_suffix.empty()) && (m.pretok != PT_CLIP || !m.bpe_prefix.empty()))
        throw Unsupported("byte-level BPE with continuing_subword_prefix / end_of_word_suffix (an end_of_word_suffix is on the path behind the CLIP "
                          "pre-tokenizer alone, with no continuing_subword_prefix)");
    if (m.byte_level && m.byte_fallback) throw Unsupported("byte-level BPE with byte_fallback");
    if (m.pretok == PT_CLIP) {
        if (m.bpe_suffix.empty()) throw Unsupported("pre_tokenizer: the CLIP Split + ByteLevel in front of a BPE without end_of_word_suffix is outside the hot path");
        if (m.bpe_suffix.size() > 31) throw Unsupported("BPE continuing_subword_prefix / end_of_word_suffix longer than 31 bytes");
        // (vocab.get(sequence) would look the text up without the suffix its entry carries: not built)
        if (m.ignore_merges) throw Unsupported("byte-level BPE with end_of_word_suffix and ignore_merges");
        m.byte_suffix = true;
    }
    if (m.char_bpe) build_char_ids(v, m);
    if (m.byte_level) build_byte_ids(v, m);
    parse_merges(v, m);
}

// WordPiece and WordLevel: over characters alone; each names its unk token, with its own default
void parse_wordpiece_or_wordlevel(const Vocab& v, HostModel& m) {
    const bool wp = v.mtype == "WordPiece";
    m.model = wp ? MODEL_WORDPIECE : MODEL_WORDLEVEL;
    if (m.byte_level) throw Unsupported(v.mtype + " behind ByteLevel");
    m.unk_token = v.model->get_str("unk_token", wp ? "[UNK]" : "<unk>");
    if (wp) m.cont_prefix = v.model->get_str("continuing_subword_prefix", "##");
    if (wp) m.max_input_chars = (uint32_t)v.model->get_num("max_input_chars_per_word", 100);
    lookup_unk(v, m);
}

// Unigram (models/unigram/model.rs): a Viterbi search per pre-token over f64 scores (unigram_core.hpp, kernels/unigram.hip).  On the
// path behind Metaspace(split = true) alone: the front's other layouts cut a piece into units, and a comparison of prefix + score
// sums made on a unit alone can round differently from the reference's, made over the whole piece.
// reads the Unigram options, pretok, norm, ms_split (and the pre-tokenizer's type, for a message); writes model, the unk fields,
// byte_fallback, byte_id, uni_bytes.  check_layout skips the U+2581 front's BPE questions for this model.
void parse_unigram(const JsonValue* root, const Vocab& v, HostModel& m) {
    m.model = MODEL_UNIGRAM;
    if (m.pretok != PT_METASPACE)
        throw Unsupported("model: Unigram (a vocab of scored pieces) is on the path behind Metaspace(split = true) only; pre_tokenizer '" +
                          type_name_or_null(root->get("pre_tokenizer")) + "' is not");
    if ((m.norm != NORM_NONE && m.norm != NORM_PRECOMPILED && m.norm != NORM_NFKC) || !m.ms_split)
        throw Unsupported("model: Unigram (a vocab of scored pieces) over whole pieces -- Metaspace(split = false), or a null pre_tokenizer behind the U+2581 "
                          "normalizers -- is outside the hot path: the front cuts such a piece into units, and the reference compares f64 sums of "
                          "prefix + score over the whole piece, which a unit alone can round differently (only Metaspace(split = true) is on the path)");
    const JsonValue* uk = v.model->get("unk_id");
    if (uk && uk->is_number()) {
        if (uk->num < 0 || uk->num >= (double)v.uni_pieces.size()) throw Unsupported("model: Unigram unk_id " + std::to_string((long long)uk->num) + " is beyond the vocab (UnkIdNotInVocabulary)");
        m.has_unk = true;
        m.unk_id = (uint32_t)uk->num;
        m.unk_token = v.uni_pieces[m.unk_id];
    }
    m.byte_fallback = v.model->get_bool("byte_fallback", false);
    for (int b = 0; b < 256; ++b) m.byte_id[b] = CHAR_NONE;
    if (m.byte_fallback) {
        // a run the vocabulary lacks becomes the <0xXX> tokens of its bytes only if ALL of them exist (unigram/model.rs:453-468: per
        // run in the reference; every byte of valid UTF-8 but 0xC0, 0xC1, 0xF5.. can occur, so the flag asks for all 256 and a file
        // that lacks one keeps its unk runs -- what the reference does for every run that holds such a byte; the others are refused)
        int have = 0;
        for (int b = 0; b < 256; ++b)
            if (const uint32_t* id = byte_token_id(v, b)) { m.byte_id[b] = *id; ++have; }
        m.uni_bytes = have == 256;
        if (have != 0 && have != 256)
            throw Unsupported("model: Unigram byte_fallback with " + std::to_string(have) + " of the 256 <0xXX> pieces (all or none are on the path)");
    }
    if (v.id.count("")) throw Unsupported("model: Unigram vocab with an empty piece is outside the hot path");
    // (the offsets of a byte-fallback run are put together from the result itself, kernels/unigram.hip k_unigram_run_offsets: no run may
    // begin with the U+2581 that opens a pre-token, which holds when U+2581 is a piece and the unk piece does not begin with one)
    if (m.uni_bytes && (!v.id.count(kMetaspace) || (m.has_unk && m.unk_token.compare(0, 3, kMetaspace) == 0)))
        throw Unsupported("model: Unigram byte_fallback with a vocab that lacks the piece U+2581 (or whose unk piece begins with it) is outside the hot path");
}

// picks the model's parser by v.mtype (read_vocab resolved it); the last refusal is for a type nothing here knows
void parse_model(const JsonValue* root, const Vocab& v, HostModel& m) {
    if (v.mtype == "BPE") parse_bpe(v, m);
    else if (v.mtype == "WordPiece" || v.mtype == "WordLevel") parse_wordpiece_or_wordlevel(v, m);
    else if (v.unigram) parse_unigram(root, v, m);
    else throw Unsupported("model: type '" + v.mtype + "' is outside the hot path");
}

// ---- 13. normalizer x pre-tokenizer x model: what each component accepted alone but the three are not built for together ----
// reads norm, pretok, model and their options, added_tokens, v.id; writes nothing.  IN THIS ORDER -- a file these questions apply to two
// of gets the first one's words -- and behind every refusal of the components' own parsers.
void check_layout(const Vocab& v, const HostModel& m) {
    if (m.pretok == PT_METASPACE && m.model != MODEL_UNIGRAM) {
        if (m.model != MODEL_BPE || !m.char_bpe)
            throw Unsupported("pre_tokenizer: the U+2581 front (Metaspace, or null behind the U+2581 normalizers) is only on the path in front of BPE over characters");
        if (!m.bpe_prefix.empty() || !m.bpe_suffix.empty())
            throw Unsupported("pre_tokenizer: the U+2581 front with continuing_subword_prefix / end_of_word_suffix");
        if (!m.ms_split) {
            // (the device cuts every piece at each U+2581 behind another char: exact by parse_merges' check, if the vocabulary has the U+2581
            // symbol itself -- and not for ignore_merges, whose whole-word lookup is of the whole piece)
            if (m.ignore_merges) throw Unsupported("pre_tokenizer: ignore_merges over whole pieces (no split at U+2581) is outside the hot path");
            if (v.id.find(kMetaspace) == v.id.end()) throw Unsupported("pre_tokenizer: whole-piece BPE (no split at U+2581) with a vocabulary that lacks U+2581 is outside the hot path");
        }
    }
    if (m.norm == NORM_NFC &&
        !(m.model == MODEL_BPE && !m.char_bpe && (m.pretok == PT_BYTELEVEL_GPT2 || m.pretok == PT_LLAMA3 || m.pretok == PT_SPLIT_CHAIN || m.pretok == PT_DIGITS_GPT2 ||
                                                  m.pretok == PT_BYTELEVEL_NOREGEX || m.pretok == PT_CLIP)))
        throw Unsupported("normalizer: NFC is only on the path in front of byte-level BPE (ByteLevel, or a Split of the tiktoken family + ByteLevel); "
                          "in front of BPE over characters, WordPiece, WordLevel or the U+2581 front it is not");
    if (m.norm == NORM_CHAIN && !(m.model == MODEL_WORDPIECE || m.model == MODEL_WORDLEVEL || (m.model == MODEL_BPE && m.char_bpe)))
        throw Unsupported(chain_refusal(m, "this model"));
    // (the same refusal every encode call makes for any normalizer, made at load for this one: the file can never encode)
    if (m.norm == NORM_NFC && m.byte_level && m.add_prefix_space) throw Unsupported("ByteLevel add_prefix_space behind a normalizer (NFC)");
    // (NFKC: in front of the U+2581 front and one of its two models; everything else keeps the words the type was always refused by)
    if (m.norm == NORM_NFKC && !(m.pretok == PT_METASPACE && (m.model == MODEL_UNIGRAM || (m.model == MODEL_BPE && m.char_bpe))))
        throw Unsupported("normalizer: type 'NFKC' is outside the hot path");
    if (m.norm == NORM_PRECOMPILED) {
        if (m.model != MODEL_UNIGRAM) throw Unsupported("normalizer: Precompiled is only on the path in front of a Unigram model");
        for (const AddedToken& a : m.added_tokens)
            if (a.normalized) throw Unsupported("added token '" + a.content + "' is normalized = true behind the Precompiled normalizer (matched on the normalized text: not on the path)");
    }
    if (m.norm == NORM_METASPACE)
        for (const AddedToken& a : m.added_tokens)
            if (a.normalized) throw Unsupported("added token '" + a.content + "' is normalized = true behind the U+2581 normalizer (matched on the normalized text: not on the path)");
}

// ---- 14. BPE with an end_of_word_suffix: the whole-word candidates lose it ----
// BPE over characters with an end_of_word_suffix: the vocabulary entry of a WHOLE word carries the suffix its text does not.  The
// whole-word table (build_word_tables) is keyed by text: the merge-stable shortcut's candidates are the entries minus their suffix (an
// entry without it cannot be a word's last symbol, let alone the whole word) -- each is then run through the device's merge kernel and
// only kept if the result is exactly its own id (capi/tables.cpp verify_direct_words).  ignore_merges looks the TEXT up as it stands
// (vocab.get(sequence), bpe/model.rs:559-567): no stripping there.
// Byte-level BPE with a suffix (behind PT_CLIP) alike: raw_tokens are the entries' raw bytes, so the suffix is taken off in its raw form.
// reads the BPE options; rewrites raw_tokens in place (an entry that is no candidate becomes "", which the table builders skip)
void strip_suffix_from_raw_tokens(const Vocab& v, HostModel& m) {
    if (!((m.char_bpe || m.byte_suffix) && !m.ignore_merges && !m.bpe_suffix.empty())) return;
    std::string sfx = m.bpe_suffix;
    if (m.byte_suffix && !bytelevel_to_raw(m.bpe_suffix, v.c2b, &sfx))
        throw Unsupported("byte-level BPE with an end_of_word_suffix that holds a char outside the byte-level alphabet");
    for (std::string& r : m.raw_tokens) {
        if (r.size() > sfx.size() && r.compare(r.size() - sfx.size(), sfx.size(), sfx) == 0) r.resize(r.size() - sfx.size());
        else r.clear();
    }
    // (two entries may now share a text -- "ab</w>" and a stray "ab</w></w>" -- : the table wants distinct keys, the first one stays)
    std::unordered_map<std::string, size_t> seen;
    for (size_t i = 0; i < m.raw_tokens.size(); ++i)
        if (!m.raw_tokens[i].empty() && !seen.emplace(m.raw_tokens[i], i).second) m.raw_tokens[i].clear();
}

// ---- 15. the tables keyed by the vocabulary's raw bytes ----
// whole-word tables (BPE: ignore_merges + merge-stable shortcut; WordLevel: the model; WordPiece: the longest candidate piece is the
// whole word, so a whole-word hit ends the match at once; Unigram: a whole-word hit is final only where the Viterbi of that word alone
// yields [id] -- proved on the device at load).  reads raw_tokens / raw_ids in order; writes word_table, long_*, n_words
void build_word_tables(HostModel& m) {
    std::vector<WordSlot> words;
    m.long_off.push_back(0);
    for (size_t i = 0; i < m.raw_tokens.size(); ++i) {
        const std::string& r = m.raw_tokens[i];
        if (r.empty()) continue;
        if (r.size() <= (size_t)WORD_MAX_KEY) {
            uint8_t buf[16] = {0};
            memcpy(buf, r.data(), r.size());
            WordSlot s{};
            memcpy(&s.lo, buf, 8);
            memcpy(&s.hi, buf + 8, 8);
            s.len = (uint32_t)r.size();
            s.id = m.raw_ids[i];
            s.flags = 0;
            words.push_back(s);
        } else {
            m.long_blob.insert(m.long_blob.end(), r.begin(), r.end());
            m.long_off.push_back((uint32_t)m.long_blob.size());
            m.long_id.push_back(m.raw_ids[i]);
        }
    }
    m.n_words = (uint32_t)words.size();
    build_word_table(m, words);
    build_long_table(m);
}

// the byte trie of WordPiece (two roots: word-initial pieces, continuation pieces without their prefix) and of Unigram (every piece under
// root 0: the reference's common_prefix_search, unigram/model.rs:285-288).  reads raw_tokens / raw_ids in order, cont_prefix; writes trie
void build_model_trie(HostModel& m) {
    if (m.model != MODEL_WORDPIECE && m.model != MODEL_UNIGRAM) return;
    std::vector<std::pair<std::string, uint32_t>> ini, cont;
    for (size_t i = 0; i < m.raw_tokens.size(); ++i) {
        const std::string& r = m.raw_tokens[i];
        if (r.empty()) continue;
        ini.emplace_back(r, m.raw_ids[i]);
        if (m.model != MODEL_WORDPIECE) continue;
        if (!m.cont_prefix.empty() && r.size() > m.cont_prefix.size() && r.compare(0, m.cont_prefix.size(), m.cont_prefix) == 0)
            cont.emplace_back(r.substr(m.cont_prefix.size()), m.raw_ids[i]);
        else if (m.cont_prefix.empty())
            cont.emplace_back(r, m.raw_ids[i]);
    }
    build_trie(m, ini, cont);
}

// ---- 16. the class tables and the normalizer's tables ----
// reads norm, nfc_lower, chain, pretok; writes uc_*, bn_*, nfc_*, nfk_* (build_added_patterns normalizes through them)
void build_normalizer_tables(HostModel& m) {
    build_unicode(m);
    if (m.norm == NORM_BERT) build_bert_norm(m);
    if (m.norm == NORM_NFC) build_nfc_tables(m);
    if (m.nfc_lower) build_norm_chain(m, {CHAIN_LOWERCASE});        // (to_lowercase alone in the chain's layout, as NFD's modes have it)
    if (m.norm == NORM_NFKC) build_nfkc_tables(m);
    if (m.norm == NORM_CHAIN && !m.nfd_mode()) build_norm_chain(m, m.chain);
    if (m.nfd_mode()) {                                      // (the NFC normalizer's tables, and to_lowercase alone in the chain's layout)
        build_nfc_tables(m);
        if (m.chain_has(CHAIN_LOWERCASE)) build_norm_chain(m, {CHAIN_LOWERCASE});
    }
}

// ---- 17. AddedVocabulary pattern sets ----
// Replace(Regex "\\s+" -> " ") of the CLIP chain: every \s run of a pattern is one ' '
std::string fold_whitespace_runs(const HostModel& m, const std::string& pat) {
    std::string folded;
    bool in_run = false;
    for (size_t i = 0; i < pat.size();) {
        uint32_t cp = 0;
        const int l = std::max(1, utf8_decode((const uint8_t*)pat.data() + i, pat.size() - i, &cp));
        const bool ws = uc_flags(m, cp) & UC_RX_S;
        if (!ws) folded.append(pat, i, (size_t)l);
        else if (!in_run) folded.push_back(' ');
        in_run = ws;
        i += (size_t)l;
    }
    return folded;
}

// the pattern of a normalized added token: its content through the file's normalizer.  Each normalizer refuses in its own words what
// its core does not build; false: the token normalizes to nothing, and the automaton has nothing to match.  (NFC keeps even an empty
// pattern -- it never makes one of a non-empty content -- and alone folds the CLIP chain's whitespace.)
bool normalized_pattern(const HostModel& m, const AddedToken& a, std::string* pat) {
    bool refused = false;
    const char* form = nullptr;
    if (m.norm == NORM_BERT) *pat = m.bert_normalize(a.content, &refused);
    else if (m.norm == NORM_CHAIN) { *pat = m.chain_normalize(a.content, nullptr, &refused); form = "NFD"; }
    else if (m.norm == NORM_NFC) { *pat = m.nfc_normalize(a.content, nullptr, &refused); form = "NFC"; }
    else if (m.norm == NORM_NFKC) { *pat = m.nfkc_normalize(a.content, nullptr, &refused); form = "NFKC"; }
    else return true;
    if (refused && !form) throw Unsupported("added token '" + a.content + "' holds a character whose NFD reordering is context dependent");
    if (refused) throw Unsupported("added token '" + a.content + "' holds a run of more than 48 combining characters (" + form + " of such a run is not built)");
    if (m.norm != NORM_NFC) return !pat->empty();
    if (m.nfc_ws_fold) *pat = fold_whitespace_runs(m, *pat);
    return true;
}

// reads added_tokens and the normalizer's tables (normalized tokens match by their normalized form); writes at[0], at[1]
void build_added_patterns(HostModel& m) {
    struct Pat { std::string s; uint32_t id, flags; };
    std::vector<Pat> pats[2];
    // the automaton is built over the special tokens first, then the others, each in the order they were added
    // (refresh_added_tokens, added_vocabulary.rs:379-399): of two tokens with one pattern -- "Ab" and "AB" behind a lowercasing
    // normalizer -- the first in THAT order is the one a match reports
    std::vector<const AddedToken*> order;
    for (int pass = 0; pass < 2; ++pass)
        for (const AddedToken& a : m.added_tokens)
            if ((pass == 0) == a.special) order.push_back(&a);
    for (const AddedToken* ap : order) {
        const AddedToken& a = *ap;
        if (a.content.empty()) continue;                       // add_tokens ignores empty contents (added_vocabulary.rs:288-291)
        std::string pat = a.content;
        if (a.normalized && !normalized_pattern(m, a, &pat)) continue;
        pats[a.normalized ? 1 : 0].push_back(Pat{pat, a.id, (a.single_word ? 1u : 0u) | (a.lstrip ? 2u : 0u) | (a.rstrip ? 4u : 0u) | (a.special ? 8u : 0u)});
    }
    for (int c = 0; c < 2; ++c) {
        std::vector<Pat>& ps = pats[c];
        // equal patterns: the first one in the automaton's order is reported
        std::stable_sort(ps.begin(), ps.end(), [](const Pat& x, const Pat& y) { return x.s < y.s; });
        std::vector<Pat> uniq;
        for (const Pat& p : ps) { if (uniq.empty() || uniq.back().s != p.s) uniq.push_back(p); }
        HostModel::PatternSet& S = m.at[c];
        S.first.assign(257, 0);
        S.off.push_back(0);
        for (const Pat& p : uniq) {
            S.first[(uint8_t)p.s[0] + 1]++;
            S.blob.insert(S.blob.end(), p.s.begin(), p.s.end());
            S.off.push_back((uint32_t)S.blob.size());
            S.id.push_back(p.id);
            S.flags.push_back(p.flags);
        }
        for (int b = 0; b < 256; ++b) S.first[b + 1] += S.first[b];
    }
}

}  // namespace

// The load, as its table of contents.  Every stage says in its header what it reads and writes; the order is the order of the refusals
// and of the tables' layout (see the top of this part).
HostModel HostModel::from_json(const char* json, size_t len) {
    JsonPtr root_owner;
    try {
        root_owner = json_parse(json, len);
    } catch (const std::exception& e) {
        throw Invalid(e.what());
    }
    const JsonValue* root = root_owner.get();
    if (!root->is_object()) throw Invalid("tokenizer.json: top level is not an object");
    HostModel m;
    std::fill(m.byte_id, m.byte_id + 256, 0xFFFFFFFFu);

    parse_truncation_padding(root, m);
    parse_normalizer(root, m);
    check_normalizer_against_pretok_type(root, m);
    m.pretok = parse_pretok(root->get("pre_tokenizer"), m);
    finish_pretok(m);
    parse_post_processor(root, m);
    parse_added_tokens(root, m);

    Vocab v;
    read_vocab(root, m, v);
    assign_added_token_ids(v, m);
    build_raw_tokens(v, m);
    build_decode_tables(m, root, v.id, v.c2b, v.unigram ? &v.uni_pieces : nullptr);
    parse_model(root, v, m);
    check_layout(v, m);

    strip_suffix_from_raw_tokens(v, m);
    build_word_tables(m);
    build_model_trie(m);
    build_normalizer_tables(m);
    build_added_patterns(m);
    return m;
}

int HostModel::bn_expand_cp(uint32_t cp, uint32_t* out, int* refused) const {
    constexpr uint32_t DROP = 1, WS = 2, CJK = 4, REORDER = 8, D = 16, LC = 32;     // bert_norm_tables.inc flag bits
    auto flags = [&](uint32_t c) -> uint32_t { return c >= 0x110000u ? 0u : bn_stage2[((uint32_t)bn_stage1[c >> 8] << 8) | (c & 255u)]; };
    auto lookup = [&](uint32_t c, uint32_t kind, uint32_t* o) -> int {
        const MergeSlot& x = bn_map[merge_hash1(c, kind, bn_seed) & bn_mask];
        const MergeSlot& y = bn_map[merge_hash2(c, kind, bn_seed) & bn_mask];
        const MergeSlot* hit = (x.a == c && x.b == kind) ? &x : (y.a == c && y.b == kind) ? &y : nullptr;
        if (!hit) { o[0] = c; return 1; }
        const unsigned long long v = ((unsigned long long)hit->new_id << 32) | hit->rank;
        int k = 0;
        const uint32_t a = (uint32_t)(v & 0x1FFFFFu), c1 = (uint32_t)((v >> 21) & 0x1FFFFFu), c2 = (uint32_t)((v >> 42) & 0x1FFFFFu);
        if (a != 0x1FFFFFu) o[k++] = a;
        if (c1 != 0x1FFFFFu) o[k++] = c1;
        if (c2 != 0x1FFFFFu) o[k++] = c2;
        return k;
    };
    *refused = 0;
    uint32_t f = flags(cp);
    if (bn_clean_text) {
        if (f & DROP) return 0;
        if (f & WS) { cp = ' '; f = 0; }
    }
    int k = 0;
    const bool cjk = bn_handle_chinese && (f & CJK);
    if (cjk) out[k++] = ' ';
    uint32_t seq[3] = {cp, 0, 0};
    int n1 = 1;
    if (bn_strip_accents) {
        if (f & REORDER) *refused = 1;
        if (f & D) n1 = lookup(cp, 0, seq);
    }
    for (int q = 0; q < n1; ++q) {
        const uint32_t y = seq[q];
        if (bn_lowercase && (flags(y) & LC)) k += lookup(y, 1, out + k);
        else out[k++] = y;
    }
    if (cjk) out[k++] = ' ';
    return k;
}

int HostModel::chain_expand_cp(uint32_t cp, uint32_t* out) const {
    if (!(bn_core_flags(bn_stage1.data(), bn_stage2.data(), cp) & 1u)) { out[0] = cp; return 1; }
    const BnCoreTables ct{bn_stage1.data(), bn_stage2.data(), bn_map.data(), bn_mask, bn_seed, false};
    uint32_t lo = 0, hi = 0;
    if (!bn_core_map(ct, cp, 0u, &lo, &hi)) { out[0] = cp; return 1; }
    const unsigned long long v = ((unsigned long long)hi << 32) | lo;
    int k = 0;
    for (int q = 0; q < 3; ++q) {
        const uint32_t c = (uint32_t)((v >> (21 * q)) & 0x1FFFFFu);
        if (c != 0x1FFFFFu) out[k++] = c;
    }
    return k;
}

std::string HostModel::chain_normalize(const std::string& s, std::vector<uint32_t>* norig, bool* refused) const {
    if (nfd_mode()) return nfc_normalize(s, norig, refused);
    std::string out;
    int64_t i = 0;
    const int64_t n = (int64_t)s.size();
    while (i < n) {
        uint32_t len;
        const uint32_t cp = bn_core_decode((const uint8_t*)s.data(), i, n, &len);
        uint32_t o[3];
        const int k = ((uint8_t)s[i] & 0xC0u) == 0x80u ? 0 : chain_expand_cp(cp, o);      // (a stray continuation byte has no output, as in k_bn_count)
        const size_t before = out.size();
        for (int q = 0; q < k; ++q) {
            uint8_t b[4];
            out.append((const char*)b, nfc_utf8_put(b, o[q]));
        }
        if (norig) norig->insert(norig->end(), out.size() - before, (uint32_t)i);
        i += len;
    }
    return out;
}

void HostModel::build_nfc() { build_nfc_tables(*this); }
void HostModel::build_nfkc() { build_nfkc_tables(*this); }

// The charsmap of a Precompiled normalizer (precompiled_core.hpp for the layout).  Everything the device will ever index is checked here:
// the sizes, the replacement strings (UTF-8, NUL-terminated), and every unit a key's walk can reach from the root -- its next position,
// its value's position and the value itself -- so a blob the reference would panic on is refused, not probed.
void HostModel::set_precompiled(const std::string& blob) {
    const char* const bad = "normalizer: Precompiled precompiled_charsmap is malformed: ";
    if (blob.empty()) throw Unsupported("normalizer: Precompiled with an empty precompiled_charsmap");
    if (blob.size() < 8) throw Unsupported(std::string(bad) + "shorter than its header and one unit");
    auto le32 = [&](size_t at) { return (uint32_t)(uint8_t)blob[at] | ((uint32_t)(uint8_t)blob[at + 1] << 8) | ((uint32_t)(uint8_t)blob[at + 2] << 16) | ((uint32_t)(uint8_t)blob[at + 3] << 24); };
    const uint32_t trie_bytes = le32(0);
    if (trie_bytes < 4u || (trie_bytes & 3u) || (size_t)trie_bytes > blob.size() - 4) throw Unsupported(std::string(bad) + "trie size " + std::to_string(trie_bytes) + " of a blob of " + std::to_string(blob.size()) + " bytes");
    const uint32_t n = trie_bytes / 4u;
    pc_units.resize(n);
    for (uint32_t k = 0; k < n; ++k) pc_units[k] = le32(4 + 4 * (size_t)k);
    pc_rep.assign(blob.begin() + 4 + trie_bytes, blob.end());
    if (pc_rep.empty() || pc_rep.back() != 0u) pc_rep.push_back(0u);        // (the crate reads a replacement up to a NUL or the blob's end)
    for (size_t i = 0; i < pc_rep.size();) {                                 // the crate holds them as one str: UTF-8
        const uint32_t b0 = pc_rep[i];
        const uint32_t l = b0 < 0x80u ? 1u : (b0 >= 0xC2u && b0 < 0xE0u) ? 2u : (b0 >= 0xE0u && b0 < 0xF0u) ? 3u : (b0 >= 0xF0u && b0 < 0xF5u) ? 4u : 0u;
        bool ok = l != 0u && i + l <= pc_rep.size();
        for (uint32_t k = 1; ok && k < l; ++k) ok = (pc_rep[i + k] & 0xC0u) == 0x80u;
        if (ok && l == 3u) ok = !(b0 == 0xE0u && pc_rep[i + 1] < 0xA0u) && !(b0 == 0xEDu && pc_rep[i + 1] >= 0xA0u);
        if (ok && l == 4u) ok = !(b0 == 0xF0u && pc_rep[i + 1] < 0x90u) && !(b0 == 0xF4u && pc_rep[i + 1] >= 0x90u);
        if (!ok) throw Unsupported(std::string(bad) + "the replacement strings are not UTF-8 (byte " + std::to_string(i) + ")");
        i += l;
    }
    auto offset_of = [](uint32_t u) { return (u >> 10) << ((u & 0x200u) >> 6); };
    for (int q = 0; q < 4; ++q) pc_first[q] = 0ull;
    pc_growth = 1;
    struct Node { uint32_t pos, depth; };
    std::vector<Node> stack;
    std::vector<uint8_t> seen(n, 0);
    const uint32_t root = offset_of(pc_units[0]);
    if (root >= n) throw Unsupported(std::string(bad) + "the root points outside the array");
    stack.push_back({root, 0u});
    seen[root] = 1;
    // (darts-clone builds from a DAWG: two units may lead to one node.  The walk is breadth first, so a node is first reached -- and its
    // leaves' growth taken -- at the SMALLEST depth any key reaches it at: the bound holds whichever path a text takes)
    for (size_t head = 0; head < stack.size(); ++head) {
        const Node nd = stack[head];
        for (uint32_t c = 1; c < 256u; ++c) {
            const uint32_t p = nd.pos ^ c;
            if (p >= n) continue;                                            // (the device reads no unit there: no match)
            const uint32_t u = pc_units[p];
            if ((u & 0x800000FFu) != c) continue;
            const uint32_t next = p ^ offset_of(u);
            if (next >= n) throw Unsupported(std::string(bad) + "unit " + std::to_string(p) + " points outside the array");
            if (nd.depth == 0u) pc_first[c >> 6] |= 1ull << (c & 63u);
            if ((u >> 8) & 1u) {
                const uint32_t v = pc_units[next] & 0x7FFFFFFFu;
                if (v >= pc_rep.size()) throw Unsupported(std::string(bad) + "the value of unit " + std::to_string(next) + " lies outside the replacement strings");
                uint32_t e = v;
                while (pc_rep[e] != 0u) ++e;
                if (e - v > PC_REP_MAX) throw Unsupported("normalizer: Precompiled with a replacement of " + std::to_string(e - v) + " bytes (at most " + std::to_string(PC_REP_MAX) + " are on the path)");
                pc_growth = std::max(pc_growth, (e - v + nd.depth) / (nd.depth + 1u));
            }
            if (!seen[next] && nd.depth < 64u) { seen[next] = 1; stack.push_back({next, nd.depth + 1u}); }
        }
    }
    two_stage(flat_of(kGcRuns), &gc_stage1, &gc_stage2);
}

std::string HostModel::precompiled_normalize(const std::string& s, std::vector<uint32_t>* norig) const {
    PcTables t{pc_units.data(), (uint32_t)pc_units.size(), pc_rep.data(), (uint32_t)pc_rep.size(), gc_stage1.data(), gc_stage2.data(), {pc_first[0], pc_first[1], pc_first[2], pc_first[3]}};
    const int64_t n = (int64_t)s.size();
    std::vector<nfc_mask_t> bound((size_t)(n >> 6) + 2, 0ull);
    bound[0] = 1ull;                                       // one piece
    std::string padded = s;
    padded.append(8, '\0');
    const uint8_t* text = (const uint8_t*)padded.data();
    std::string out;
    if (norig) norig->clear();
    const uint32_t lost = pc_lost_chars(t, text, n, bound.data(), 0);
    for (int64_t p = 0; p < n;) {
        uint32_t l, ro = 0, rl = 0;
        int64_t se = 0;
        nfc_decode(text, n, p, &l);
        const PcOut k = pc_char_out(t, text, n, bound.data(), p, &ro, &rl, &se);
        if (k == PC_COPY) {
            out.append(s, (size_t)p, l);
            if (norig) norig->insert(norig->end(), l, (uint32_t)pc_chars_back(text, n, p, lost));
        } else if (k == PC_REP) {
            int64_t q = p;                                  // the source char the replacement's next char takes
            bool inserted = false;                          // ... which is beyond the last source char
            for (uint32_t z = 0; z < rl;) {
                uint32_t cl, ql;
                nfc_decode(t.rep + ro, rl, z, &cl);
                out.append((const char*)t.rep + ro + z, cl);
                z += cl;
                const int64_t src = (inserted && z == rl && pc_tail_moves(t, text, n, bound.data(), se)) ? se : q;
                if (norig) norig->insert(norig->end(), cl, (uint32_t)pc_chars_back(text, n, src, lost));
                nfc_decode(text, n, q, &ql);
                if (q + ql < se) q += ql; else inserted = true;
            }
        }
        p += l;
    }
    return out;
}

namespace {
template <bool K>
std::string nfc_normalize_piece(const NfcTables& t, const std::string& s, std::vector<uint32_t>* norig, bool* refused);
}

std::string HostModel::nfkc_normalize(const std::string& s, std::vector<uint32_t>* norig, bool* refused) const {
    NfcTables t{nfc_stage1.data(), nfc_stage2.data(), nfc_map.data(), nfc_mask, nfc_seed};
    t.lmap = nfk_map.data(); t.lmap_mask = nfk_mask; t.lmap_seed = nfk_seed; t.kflat = nfk_flat.data();      // (K mode's slots, nfc_core.hpp)
    return nfc_normalize_piece<true>(t, s, norig, refused);
}

std::string HostModel::nfc_normalize(const std::string& s, std::vector<uint32_t>* norig, bool* refused) const {
    NfcTables t{nfc_stage1.data(), nfc_stage2.data(), nfc_map.data(), nfc_mask, nfc_seed};
    if ((t.mode = nfc_mode()) & NFC_ANY_LOWER) { t.l1 = bn_stage1.data(); t.l2 = bn_stage2.data(); t.lmap = bn_map.data(); t.lmap_mask = bn_mask; t.lmap_seed = bn_seed; }
    return nfc_normalize_piece<false>(t, s, norig, refused);
}

namespace {
template <bool K>
std::string nfc_normalize_piece(const NfcTables& t, const std::string& s, std::vector<uint32_t>* norig, bool* refused) {
    const int64_t n = (int64_t)s.size();
    std::vector<nfc_mask_t> bound((size_t)(n >> 6) + 2, 0ull);
    bound[0] = 1ull;                                       // one piece
    const uint8_t* text = (const uint8_t*)s.data();
    std::string out;
    if (norig) norig->clear();
    NfcSeg g;
    int64_t p = 0;
    while (p < n) {
        uint32_t l;
        const uint32_t f = nfc_flags(t, nfc_decode(text, n, p, &l));
        if (nfc_trivial<K>(t, text, n, bound.data(), p, f, l)) {
            out.append(s, (size_t)p, l);
            if (norig) norig->insert(norig->end(), l, (uint32_t)p);
            p += l;
            continue;
        }
        if (!nfc_segment<K>(t, text, n, bound.data(), p, g)) {
            if (refused) *refused = true;
            return out;
        }
        for (int k = 0; k < g.n; ++k) {
            uint8_t b[4];
            const uint32_t bl = nfc_utf8_put(b, g.cp[k]);
            out.append((const char*)b, bl);
            if (norig) norig->insert(norig->end(), bl, (uint32_t)p + g.al[k]);
        }
        p = g.e;
    }
    return out;
}
}  // namespace

std::string HostModel::bert_normalize(const std::string& s, bool* refused) const {
    std::string out;
    size_t i = 0;
    while (i < s.size()) {
        const uint8_t b0 = (uint8_t)s[i];
        uint32_t cp, len;
        auto cb = [&](size_t k) -> uint32_t { return i + k < s.size() ? ((uint8_t)s[i + k] & 0x3Fu) : 0u; };
        if (b0 < 0x80u) { cp = b0; len = 1; }
        else if (b0 < 0xE0u) { cp = ((b0 & 0x1Fu) << 6) | cb(1); len = 2; }
        else if (b0 < 0xF0u) { cp = ((b0 & 0x0Fu) << 12) | (cb(1) << 6) | cb(2); len = 3; }
        else { cp = ((b0 & 0x07u) << 18) | (cb(1) << 12) | (cb(2) << 6) | cb(3); len = 4; }
        const size_t at = i;
        i += len;
        uint32_t o[12];
        int r = 0;
        const int n = bn_expand_cp(cp, o, &r);
        // (a character NFD's canonical ordering could move: fine as long as it is alone in its run, bert_norm_core.hpp)
        if (r && refused &&
            !bn_alone_in_run(bn_stage1.data(), bn_stage2.data(), bn_clean_text, (const uint8_t*)s.data(), 0, (int64_t)s.size(), (int64_t)at, len,
                             bn_core_flags(bn_stage1.data(), bn_stage2.data(), cp), nullptr))
            *refused = true;
        for (int q = 0; q < n; ++q) {
            uint8_t b[4];
            out.append((const char*)b, nfc_utf8_put(b, o[q]));
        }
    }
    return out;
}

}  // namespace tkamd
