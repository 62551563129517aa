// Unigram::tokenize (models/unigram/model.rs:443-477) over Unigram::encode_optimized (:255-344) for ONE pre-token: the Viterbi
// forward pass over f64 scores, the backtrack with fused unk runs, and the lookup -- by string -- of every fused run, with the
// <0xXX> fallback.  One body for the device kernels (kernels/unigram.hip) and the host (tests/harness/unigram_harness.cpp): it is
// templated on where the per-position state lives (State), where the bytes come from (Bytes) and who takes the tokens (Emit).
//
// What the reference does, restated:
//   * best[0] = 0.0.  For every start p on a char boundary, in increasing order, base = best[p]; every vocabulary piece that is a
//     prefix of the text at p, in increasing length (common_prefix_search), offers  cand = score + base  -- ONE f64 add, in that
//     operand order -- to the node at p + len, which takes (cand, p, id) if it is unset or cand > its score: strict, so of two equal
//     candidates the one met first stays -- the earliest start (:281-306).
//   * if no piece of exactly one char matched at p, an unk node of that char offers unk_score + base the same way (:307-317); with
//     unk_id null that is MissingUnkId, but only where the node would be TAKEN (the `?` sits inside the if).
//   * the score of a piece is vocab[token_to_ids[piece]].1: of two equal pieces the later id and ITS score (:293-294).
//   * backtrack from the end; consecutive nodes whose id is unk_id -- a node that matched the unk piece literally included -- are
//     fused into one string (:320-343; fuse_unk is always true for a deserialized model, :133).
//   * every token string is looked up again by string (:450): a fused run can itself be a piece (with large positive scores two unks
//     outscore the pair's own piece).  A run the vocabulary lacks: with byte_fallback and all its <0xXX> pieces present one token
//     per byte, each with the offsets of the WHOLE run (:453-468), else one unk_id token over the run (:470).
// Only double adds and compares: no float, no reassociation, nothing a compiler may contract (there is no multiply).
#pragma once
#include <cstdint>
#include <cstring>

#include "tables.hpp"

namespace tkamd {

// what the core reads of the model (pointers into HBM on the device, into the host tables in the harness)
struct UniModel {
    const MergeSlot* trie;        // byte trie over every piece as a two-choice table: (node, byte) -> (child, id of the piece ending there or 0xFFFFFFFF)
    uint32_t trie_mask, trie_seed;
    const double* score;          // [vocab] the file's f64 per id
    double unk_score;             // min over ALL scores - 10.0 (unigram/model.rs:124-131, :277)
    uint32_t unk_id, has_unk;
    const uint32_t* byte_id;      // [256] ids of the <0xXX> pieces
    uint32_t bytes_on;            // byte_fallback with all 256 of them present
};
constexpr uint32_t UNI_ID_NONE = 0xFFFFFFFFu;
constexpr uint32_t UNI_ERR_MISSING_UNK = 1u;      // what uni_encode returns when the unk node was needed and unk_id is null

TK_HD uint64_t uni_d2u(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
TK_HD double uni_u2d(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }

// one edge of the trie: two independent 16-byte slots (the WordPiece table's probe, documents.hip pair_probe2, for host and device)
TK_HD bool uni_edge(const UniModel& u, uint32_t node, uint32_t byte, uint32_t* child, uint32_t* id) {
    const MergeSlot x = u.trie[merge_hash1(node, byte, u.trie_seed) & u.trie_mask];
    const MergeSlot y = u.trie[merge_hash2(node, byte, u.trie_seed) & u.trie_mask];
    if (x.a == node && x.b == byte) { *child = x.rank; *id = x.new_id; return true; }
    if (y.a == node && y.b == byte) { *child = y.rank; *id = y.new_id; return true; }
    return false;
}

// State: the node that ENDS at byte p of the pre-token, p = 1 .. len (position 0 is best = 0.0 and lives in the core's registers)
//   void clear(p);  bool isset(p);  double score(p);  uint32_t back(p);  uint32_t id(p);
//   void set(p, double score, uint32_t back_len, uint32_t id);
//   void set_fwd(p, uint32_t end, uint32_t id);  void get_fwd(p, uint32_t* end, uint32_t* id);      -- the token that STARTS at p, written by
//   the backtrack over the score of p (no longer needed then) so that the tokens come out front to back
// Bytes: uint32_t operator()(uint32_t p): byte p of the pre-token.   Emit: void operator()(uint32_t id, uint32_t end, bool byte_token)
template <class State, class Bytes, class Emit>
TK_HD uint32_t uni_encode(const UniModel& u, uint32_t len, State& st, const Bytes& byte, Emit& emit) {
    uint32_t err = 0u;
    for (uint32_t p = 1; p <= len; ++p) st.clear(p);
    // ---- forward (:281-319)
    for (uint32_t p = 0; p < len;) {
        const double base = p ? st.score(p) : 0.0;
        const uint32_t b0 = byte(p);
        uint32_t mblen = b0 < 0x80u ? 1u : b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : 4u;
        if (mblen > len - p) mblen = len - p;      // (a pre-token is whole chars; never past its end whatever the bytes are)
        bool has_single = false;
        uint32_t node = 0u, w = p;
        while (w < len) {
            uint32_t child, id;
            if (!uni_edge(u, node, byte(w), &child, &id)) break;
            node = child;
            ++w;
            if (id != UNI_ID_NONE) {
                const double cand = u.score[id] + base;
                if (!st.isset(w) || cand > st.score(w)) st.set(w, cand, w - p, id);
                if (w - p == mblen) has_single = true;
            }
        }
        if (!has_single) {
            const uint32_t q = p + mblen;
            const double cand = u.unk_score + base;
            if (!st.isset(q) || cand > st.score(q)) {
                if (!u.has_unk) err |= UNI_ERR_MISSING_UNK;
                st.set(q, cand, mblen, u.unk_id);
            }
        }
        p += mblen;
    }
    // ---- backtrack (:320-337), leaving forward links
    uint32_t f0_end = 0u, f0_id = 0u;
    for (uint32_t e = len; e > 0u;) {
        const uint32_t l = st.back(e), id = st.id(e), s0 = e - l;
        if (s0) st.set_fwd(s0, e, id);
        else { f0_end = e; f0_id = id; }
        e = s0;
    }
    // ---- front to back: fuse the unk runs, look every run up by string, fall back to its bytes (:326-343, :447-475)
    for (uint32_t p = 0; p < len;) {
        uint32_t e = f0_end, id = f0_id;
        if (p) st.get_fwd(p, &e, &id);
        if (u.has_unk && id == u.unk_id) {
            while (e < len) {
                uint32_t e2, id2;
                st.get_fwd(e, &e2, &id2);
                if (id2 != u.unk_id) break;
                e = e2;
            }
            uint32_t node = 0u, w = p, found = UNI_ID_NONE;      // token_to_ids.get(run)
            while (w < e) {
                uint32_t child, pid;
                if (!uni_edge(u, node, byte(w), &child, &pid)) break;
                node = child;
                ++w;
                if (w == e) found = pid;
            }
            if (found != UNI_ID_NONE) emit(found, e, false);
            else if (u.bytes_on) {
                for (uint32_t k = p; k < e; ++k) emit(u.byte_id[byte(k)], k + 1u, true);
            } else emit(u.unk_id, e, false);
        } else emit(id, e, false);
        p = e;
    }
    return err;
}

}  // namespace tkamd
