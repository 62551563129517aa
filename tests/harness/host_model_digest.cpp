// What HostModel::from_json makes of a tokenizer.json, as three 64-bit digests -- the loader's own test (tests/test_host_model_outcomes.py).
//   host_model_digest [--time] PATH...          or          host_model_digest [--time] --list FILE     (one "name<TAB>path" or "path" a line)
// One line per file:  <name>\tOK\t<config>\t<content>\t<layout>   or   <name>\tUNSUPPORTED|INVALID\t<the exception's message>
// (--time: one more column, the milliseconds from_json took).  A name not given in the list is the file's base name up to its first '.'.
//   config   every field whose value follows from the file alone, whatever the order the vocabulary was walked in
//   content  what the keyed tables hold, independent of where each entry sits
//   layout   the raw bytes of everything copied to the device that depends on the iteration order of the vocabulary's std::unordered_map
//            (this libstdc++'s): not recorded, compared between two builds of host_model.cpp
// A digest is FNV-1a over fields that each carry their length in front, so no two neighbouring fields alias.
// Every field of HostModel is in one of the three; the six cuckoo seeds (merge_seed, word_seed, trie.seed, bn_seed, nfc_seed, nfk_seed) are
// layout, since a seed says where entries sit, and byte_sfx_id is read only where byte_suffix says it was written.
// Built with g++ -O2 -std=c++17 -I tokenizers_amd/csrc next to host_model.cpp: no HIP, no Python, no GPU.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "host_model.hpp"

using namespace tkamd;

namespace {

struct Digest {
    uint64_t h = 0xCBF29CE484222325ull;
    void raw(const void* p, size_t n) {
        const uint8_t* b = (const uint8_t*)p;
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
    }
    void bytes(const void* p, size_t n) { const uint64_t len = n; raw(&len, 8); if (n) raw(p, n); }
    void num(uint64_t v) { bytes(&v, 8); }
    void str(const std::string& s) { bytes(s.data(), s.size()); }
    // a vector of a type without padding (integers, MergeSlot, WordSlot, TplPiece), as its bytes
    template <class T> void vec(const std::vector<T>& v) { static_assert(std::is_trivially_copyable<T>::value, ""); bytes(v.data(), v.size() * sizeof(T)); }
    std::string hex() const { char buf[20]; snprintf(buf, sizeof buf, "%016llx", (unsigned long long)h); return buf; }
};

void pattern_set(Digest& d, const HostModel::PatternSet& s) { d.vec(s.blob); d.vec(s.off); d.vec(s.first); d.vec(s.id); d.vec(s.flags); }

std::string config_digest(const HostModel& m) {
    Digest d;
    for (uint64_t v : {(uint64_t)m.model, (uint64_t)m.pretok, (uint64_t)m.norm, (uint64_t)m.byte_level, (uint64_t)m.add_prefix_space, (uint64_t)m.trim_offsets,
                       (uint64_t)m.pp_add_prefix_space, (uint64_t)m.bn_clean_text, (uint64_t)m.bn_handle_chinese, (uint64_t)m.bn_strip_accents, (uint64_t)m.bn_lowercase})
        d.num(v);
    d.vec(m.chain); d.str(m.chain_spelling); d.str(m.nfkc_refusal);
    for (uint64_t v : {(uint64_t)m.nfc_lower, (uint64_t)m.nfc_ws_fold, (uint64_t)m.ms_prepend, (uint64_t)m.ms_split, (uint64_t)m.ignore_merges, (uint64_t)m.has_unk, (uint64_t)m.unk_id})
        d.num(v);
    d.str(m.unk_token); d.str(m.cont_prefix); d.num(m.max_input_chars);
    // the post-processor's layouts
    d.vec(m.pp_prefix); d.vec(m.pp_suffix); d.str(m.pp_unsupported); d.vec(m.pp_pair); d.str(m.pp_pair_unsupported); d.num(m.pp_roberta);
    d.vec(m.pp_prefix_ty); d.vec(m.pp_suffix_ty); d.num(m.pp_seq_ty); d.num(m.pp_single_typed); d.num(m.pp_single_refused);
    d.vec(m.pp_pair_plain); d.vec(m.pp_single); d.vec(m.pp_single_plain);
    // truncation / padding
    for (uint64_t v : {(uint64_t)m.trunc_on, (uint64_t)m.trunc_max_length, (uint64_t)m.trunc_left, (uint64_t)(int64_t)m.trunc_strategy, (uint64_t)m.trunc_stride, (uint64_t)m.pad_on,
                       (uint64_t)m.pad_fixed, (uint64_t)m.pad_length, (uint64_t)m.pad_left, (uint64_t)m.pad_multiple, (uint64_t)m.pad_id, (uint64_t)m.pad_type_id})
        d.num(v);
    d.str(m.pad_token);
    d.num(m.vocab_size); d.num(m.n_merges);
    d.num(m.added_tokens.size());
    for (const AddedToken& a : m.added_tokens) {
        d.str(a.content); d.num(a.id);
        d.num(a.special); d.num(a.single_word); d.num(a.lstrip); d.num(a.rstrip); d.num(a.normalized);
    }
    pattern_set(d, m.at[0]); pattern_set(d, m.at[1]);
    // the model's options and direct-indexed tables
    d.bytes(m.byte_id, sizeof m.byte_id);
    for (uint64_t v : {(uint64_t)m.char_bpe, (uint64_t)m.unk_configured, (uint64_t)m.fuse_unk, (uint64_t)m.byte_fallback}) d.num(v);
    d.str(m.bpe_prefix); d.str(m.bpe_suffix);
    d.num(m.byte_suffix);
    if (m.byte_suffix) d.bytes(m.byte_sfx_id, sizeof m.byte_sfx_id);
    d.vec(m.char_id);
    for (uint64_t v : {(uint64_t)m.merge_mask, (uint64_t)m.merge_bmask, (uint64_t)m.merge_newid_affine, (uint64_t)m.merge_newid_base, (uint64_t)m.word_mask, (uint64_t)m.n_words,
                       (uint64_t)m.long_mask, (uint64_t)m.trie.mask, (uint64_t)m.trie.n_nodes})
        d.num(v);
    d.vec(m.uni_score);                                     // (the f64 bit patterns)
    d.bytes(&m.uni_unk_score, 8); d.num(m.uni_bytes);
    // the normalizers' tables: static data in a fixed order behind fixed RNG seeds, so their placement too follows from the file alone
    d.vec(m.bn_stage1); d.vec(m.bn_stage2); d.vec(m.bn_map); d.num(m.bn_mask);
    d.vec(m.nfc_stage1); d.vec(m.nfc_stage2); d.vec(m.nfc_map); d.num(m.nfc_mask);
    d.vec(m.nfk_map); d.num(m.nfk_mask); d.vec(m.nfk_flat);
    d.vec(m.pc_units); d.vec(m.pc_rep); d.bytes(m.pc_first, sizeof m.pc_first); d.num(m.pc_growth); d.num(m.pc_space_runs);
    d.vec(m.gc_stage1); d.vec(m.gc_stage2);
    // decode_batch's scalars (its tables: content and layout)
    d.num((uint64_t)m.decoder); d.str(m.dec_unsupported);
    d.num(m.dec_position_dependent); d.num(m.dec_special_is_last); d.num(m.dec_dedup); d.num(m.dec_has_bytes);
    // the pre-tokenizer's class tables and rule
    d.vec(m.uc_stage1); d.vec(m.uc_stage2); d.num(m.digits_individual);
    const uint8_t rule[4] = {m.split_rule.contr, m.split_rule.letters, m.split_rule.digit_max, m.split_rule.other_tail};
    d.bytes(rule, 4);
    d.vec(m.ucc_stage1); d.vec(m.ucc_stage2);
    return d.hex();
}

std::string content_digest(const HostModel& m) {
    Digest d;
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>> merges;
    for (const MergeSlot& s : m.merge_table)
        if (s.a != MERGE_EMPTY) merges.emplace_back(s.a, s.b, s.rank, s.new_id);
    std::sort(merges.begin(), merges.end());
    d.num(merges.size());
    for (const auto& t : merges) { d.num(std::get<0>(t)); d.num(std::get<1>(t)); d.num(std::get<2>(t)); d.num(std::get<3>(t)); }
    std::vector<std::tuple<uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t>> words;
    for (const WordSlot& s : m.word_table)
        if (s.len) words.emplace_back(s.lo, s.hi, s.len, s.id, s.flags, s.pad);
    std::sort(words.begin(), words.end());
    d.num(words.size());
    for (const auto& t : words) { d.num(std::get<0>(t)); d.num(std::get<1>(t)); d.num(std::get<2>(t)); d.num(std::get<3>(t)); d.num(std::get<4>(t)); d.num(std::get<5>(t)); }
    // the long keys: through the open-addressing table, so an entry the table does not reach is not counted
    std::vector<std::pair<std::string, uint32_t>> longs;
    for (uint32_t e1 : m.long_table)
        if (e1) longs.emplace_back(std::string((const char*)m.long_blob.data() + m.long_off[e1 - 1], m.long_off[e1] - m.long_off[e1 - 1]), m.long_id[e1 - 1]);
    std::sort(longs.begin(), longs.end());
    d.num(longs.size()); d.num(m.long_id.size());
    for (const auto& kv : longs) { d.str(kv.first); d.num(kv.second); }
    std::vector<std::pair<std::string, uint32_t>> raw;
    for (size_t i = 0; i < m.raw_tokens.size(); ++i) raw.emplace_back(m.raw_tokens[i], m.raw_ids[i]);
    std::sort(raw.begin(), raw.end());
    d.num(raw.size()); d.num(m.raw_ids.size());
    for (const auto& kv : raw) { d.str(kv.first); d.num(kv.second); }
    // the trie: its nodes are numbered in the order the keys went in, so only how many edges it holds is content
    uint64_t trie_slots = 0;
    for (const MergeSlot& s : m.trie.table) trie_slots += s.a != MERGE_EMPTY;
    d.num(trie_slots);
    // the decode tables: id -> both forms' bytes and flags, the strings read through the entries
    d.num(m.dec_entry.size());
    for (size_t i = 0; i + 3 < m.dec_entry.size(); i += 4) {
        const uint32_t* e = &m.dec_entry[i];
        d.num(e[1] & ~DEC_LEN_MASK);
        if (e[1] & DEC_ABSENT) continue;
        if (e[1] & DEC_BYTE) { d.num(e[0]); d.num(e[1] & DEC_LEN_MASK); d.num(e[2]); d.num(e[3]); continue; }
        d.bytes(m.dec_blob.data() + e[0], e[1] & DEC_LEN_MASK);
        d.bytes(m.dec_blob.data() + e[2], e[3]);
    }
    return d.hex();
}

std::string layout_digest(const HostModel& m) {
    Digest d;
    d.vec(m.merge_table); d.vec(m.merge_disp); d.vec(m.word_table);
    d.vec(m.long_blob); d.vec(m.long_off); d.vec(m.long_id); d.vec(m.long_table);
    d.vec(m.trie.table); d.vec(m.dec_entry); d.vec(m.dec_blob);
    for (uint32_t s : {m.merge_seed, m.word_seed, m.trie.seed, m.bn_seed, m.nfc_seed, m.nfk_seed}) d.num(s);
    d.num(m.raw_tokens.size());
    for (const std::string& r : m.raw_tokens) d.str(r);
    d.vec(m.raw_ids);
    return d.hex();
}

std::string one_line(std::string s) {
    for (char& c : s)
        if (c == '\n' || c == '\r' || c == '\t') c = ' ';
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    bool timed = false;
    std::vector<std::pair<std::string, std::string>> files;      // (name, path)
    auto add = [&](const std::string& name, const std::string& path) {
        std::string n = name;
        if (n.empty()) {
            const size_t slash = path.find_last_of('/');
            n = path.substr(slash == std::string::npos ? 0 : slash + 1);
            n = n.substr(0, n.find('.'));
        }
        files.emplace_back(n, path);
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--time") timed = true;
        else if (a == "--list" && i + 1 < argc) {
            std::ifstream fh(argv[++i]);
            if (!fh) { fprintf(stderr, "host_model_digest: cannot read the list %s\n", argv[i]); return 2; }
            for (std::string line; std::getline(fh, line);) {
                if (line.empty()) continue;
                const size_t tab = line.find('\t');
                if (tab == std::string::npos) add("", line);
                else add(line.substr(0, tab), line.substr(tab + 1));
            }
        } else add("", a);
    }
    if (files.empty()) { fprintf(stderr, "usage: host_model_digest [--time] PATH... | --list FILE\n"); return 2; }
    for (const auto& f : files) {
        std::ifstream fh(f.second, std::ios::binary);
        if (!fh) { fprintf(stderr, "host_model_digest: cannot read %s\n", f.second.c_str()); return 2; }
        std::stringstream ss;
        ss << fh.rdbuf();
        const std::string js = ss.str();
        std::string line;
        const auto t0 = std::chrono::steady_clock::now();
        auto ms = [&] { char buf[32]; snprintf(buf, sizeof buf, "\t%.1f", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); return std::string(timed ? buf : ""); };
        try {
            const HostModel m = HostModel::from_json(js.data(), js.size());
            const std::string took = ms();
            line = "OK\t" + config_digest(m) + "\t" + content_digest(m) + "\t" + layout_digest(m) + took;
        } catch (const Unsupported& e) {
            line = "UNSUPPORTED\t" + one_line(e.what()) + ms();
        } catch (const Invalid& e) {
            line = "INVALID\t" + one_line(e.what()) + ms();
        }
        printf("%s\t%s\n", f.first.c_str(), line.c_str());
    }
    return 0;
}
