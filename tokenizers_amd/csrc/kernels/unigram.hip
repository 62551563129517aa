// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers; it is not compiled on its own).  Unigram.

// =================================================================================================
// K_unigram_all: Unigram::tokenize (models/unigram/model.rs:443-477) over encode_optimized (:255-344), one lane per QUEUED pre-token
// (the words k_lookup could not settle: a whole-word hit is final only where this very kernel proved at load that the Viterbi of the
// word alone yields [id], capi/tables.cpp verify_direct_words).  The search itself is unigram_core.hpp, the body the host harness
// runs; here is where its state lives and where its tokens go.
//   * the queues of words of <= 16 / <= 32 / <= 64 bytes: the state -- per position an f64 best score and one word id | back length << 24
//     -- in LDS, position-major with the lanes side by side (a lane's column is its own bank pair, as the merge keys of bpe.hip are
//     laid out): 12 bytes a position, 48 KB a workgroup for 256 lanes x 16, 128 lanes x 32 or 64 lanes x 64 positions (the tiers of
//     longer words leave the other lanes of their workgroups idle: a few thousand words a batch on natural text).  The words of <= 16
//     bytes sit in two registers; the trie walks never touch the text again.
//   * longer words, whatever their length (a CJK paragraph is one pre-token): the state in HBM, 16 bytes a position at the word's OWN
//     bytes of a per-text-byte array (the node that ends at byte p of the word that starts at s is entry s + p: the entries s + 1 ..
//     s + len belong to it alone, like its slots of tmp_ids), so no slab is handed out and no word is refused for its length.  One lane
//     walks such a word serially.
// The four queues share ONE launch (as k_wordpiece_all: chains of dependent trie probes, as long as the longest one).
// The tokens leave as the WordPiece kernel's do: up to four in the row (with offsets and <= 32 bytes: the boundary bytes beside them),
// a fifth spills them to tmp_ids[s + j]; token ends in tmp_end[s + j].  A <0xXX> token ends one byte behind the last: k_token_meta snaps it
// to its char, and k_unigram_run_offsets (below) widens the tokens of a run of several chars to the whole run.
// =================================================================================================
struct UniLdsState {
    uint64_t* best;      // this lane's column: entry p - 1 at best[(p - 1) * nl]
    uint32_t* pk;
    uint32_t nl;
    __device__ __forceinline__ void clear(uint32_t p) { pk[(p - 1u) * nl] = 0xFFFFFFFFu; }
    __device__ __forceinline__ bool isset(uint32_t p) const { return pk[(p - 1u) * nl] != 0xFFFFFFFFu; }
    __device__ __forceinline__ double score(uint32_t p) const { return uni_u2d(best[(p - 1u) * nl]); }
    __device__ __forceinline__ uint32_t back(uint32_t p) const { return pk[(p - 1u) * nl] >> 24; }
    __device__ __forceinline__ uint32_t id(uint32_t p) const { return pk[(p - 1u) * nl] & TOK_ID_MASK; }
    __device__ __forceinline__ void set(uint32_t p, double sc, uint32_t back_len, uint32_t id_) { best[(p - 1u) * nl] = uni_d2u(sc); pk[(p - 1u) * nl] = id_ | (back_len << 24); }
    __device__ __forceinline__ void set_fwd(uint32_t p, uint32_t end, uint32_t id_) { best[(p - 1u) * nl] = (uint64_t)end | ((uint64_t)id_ << 32); }
    __device__ __forceinline__ void get_fwd(uint32_t p, uint32_t* end, uint32_t* id_) const { const uint64_t x = best[(p - 1u) * nl]; *end = (uint32_t)x; *id_ = (uint32_t)(x >> 32); }
};
struct UniGlobalState {
    uint4* e;            // entry p of the word: {score lo, score hi, back length (0: unset), id}
    __device__ __forceinline__ void clear(uint32_t p) { e[p] = make_uint4(0u, 0u, 0u, 0u); }
    __device__ __forceinline__ bool isset(uint32_t p) const { return e[p].z != 0u; }
    __device__ __forceinline__ double score(uint32_t p) const { const uint4 x = e[p]; return uni_u2d((uint64_t)x.x | ((uint64_t)x.y << 32)); }
    __device__ __forceinline__ uint32_t back(uint32_t p) const { return e[p].z; }
    __device__ __forceinline__ uint32_t id(uint32_t p) const { return e[p].w; }
    __device__ __forceinline__ void set(uint32_t p, double sc, uint32_t back_len, uint32_t id_) { const uint64_t b = uni_d2u(sc); e[p] = make_uint4((uint32_t)b, (uint32_t)(b >> 32), back_len, id_); }
    __device__ __forceinline__ void set_fwd(uint32_t p, uint32_t end, uint32_t id_) { e[p].x = end; e[p].y = id_; }
    __device__ __forceinline__ void get_fwd(uint32_t p, uint32_t* end, uint32_t* id_) const { *end = e[p].x; *id_ = e[p].y; }
};
struct UniKeyBytes {      // a word of <= 16 bytes in two registers
    uint64_t lo, hi;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (uint32_t)((w < 8u ? lo >> (8u * w) : hi >> (8u * (w - 8u))) & 0xFFu); }
};
struct UniTextBytes {
    const uint8_t* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (uint32_t)p[w]; }
};
// the tokens of one word, in order (the WordPiece kernel's row, word_models.hip)
struct UniEmit {
    const uint8_t* text;
    uint32_t* tmp_ids;
    uint32_t* tmp_end;
    uint32_t s, len, snap;
    uint32_t j = 0u, pos = 0u, r0 = 0u, r1 = 0u, r2 = 0u, r3 = 0u;
    __device__ __forceinline__ void operator()(uint32_t id, uint32_t end, bool) {
        // (with offsets, a word of <= 32 bytes: the boundary in front of token j rides in the row's word j, results.hip row_boundary -- a
        // <0xXX> token may start inside a char, whose range it then reports)
        const uint32_t bnd = (tmp_end && len <= 32u && j) ? row_boundary(text, s, pos, snap != 0u) : 0u;
        if (j == 0u) r0 = id;
        else if (j == 1u) r1 = id | bnd;
        else if (j == 2u) r2 = id | bnd;
        else if (j == 3u) r3 = id | bnd;
        else {
            if (j == 4u) { tmp_ids[s + 1] = r1 & TOK_ID_MASK; tmp_ids[s + 2] = r2 & TOK_ID_MASK; tmp_ids[s + 3] = r3 & TOK_ID_MASK; }
            tmp_ids[s + j] = id;
        }
        if (tmp_end) tmp_end[s + j] = end;
        pos = end;
        ++j;
    }
};
__device__ __forceinline__ UniModel uni_model_of(const DevTables& t) {
    UniModel u;
    u.trie = t.trie; u.trie_mask = t.trie_mask; u.trie_seed = t.trie_seed;
    u.score = t.uni_score; u.unk_score = t.uni_unk_score;
    u.unk_id = t.unk_id; u.has_unk = t.has_unk;
    u.byte_id = t.byte_id; u.bytes_on = t.uni_bytes;
    return u;
}

constexpr int UNI_LDS_POS = 16 * 256;      // positions x lanes of every LDS tier: 16 x 256 = 32 x 128 = 64 x 64

// TIER 0 / 1 / 2: the queues of words of <= 16 / 32 / 64 bytes, state in LDS; TIER 3: longer words, state in HBM
template <int TIER>
__device__ __forceinline__ void unigram_body(const DevTables& t, const uint8_t* __restrict__ text, const QView& v, uint4* __restrict__ rows,
                                             uint32_t* __restrict__ tmp_ids, uint32_t* __restrict__ tmp_end, int* __restrict__ err, uint4* __restrict__ gstate,
                                             uint32_t block, uint32_t n_blocks, uint32_t* s_qpre, uint64_t* s_best, uint32_t* s_pk) {
    constexpr uint32_t CAP = TIER == 0 ? 16u : TIER == 1 ? 32u : 64u;
    constexpr uint32_t NL = TIER == 3 ? 256u : (uint32_t)UNI_LDS_POS / CAP;      // lanes of the workgroup that take a word
    const uint32_t n = qview_prefix(v, s_qpre);
    if (threadIdx.x >= NL) return;                                               // (no barrier behind this point)
    const UniModel u = uni_model_of(t);
    for (uint32_t item = block * NL + threadIdx.x; item < n; item += n_blocks * NL) {
        const uint32_t qpos = qview_pos(s_qpre, v.sq_cap, item);
        const QItem it = v.q[qpos];
        const uint32_t s = it.s;
        uint32_t len = qitem_len(it.len);
        if (!len) continue;
        // (the queue class bounds the length -- the LDS columns hold CAP positions; an entry beyond it would be a bug of the lookup: the batch
        // fails, nothing is written outside the column and no word is cut short silently)
        if (TIER != 3 && len > CAP) { atomicOr(err, ERR_INTERNAL); continue; }
        UniEmit emit{text, tmp_ids, tmp_end, s, len, t.uni_bytes};
        uint32_t e;
        if (TIER == 3) {
            UniGlobalState st{gstate + s};
            const UniTextBytes by{text + s};
            e = uni_encode(u, len, st, by, emit);
        } else {
            UniLdsState st{s_best + threadIdx.x, s_pk + threadIdx.x, NL};
            if (TIER == 0) {
                UniKeyBytes by;
                load_key16(text, s, len, &by.lo, &by.hi);
                e = uni_encode(u, len, st, by, emit);
            } else {
                const UniTextBytes by{text + s};
                e = uni_encode(u, len, st, by, emit);
            }
        }
        if (e & UNI_ERR_MISSING_UNK) atomicOr(err, ERR_MISSING_UNK);           // "Encountered an unknown token but `unk_id` is missing" (unigram/model.rs:315)
        const uint4 row_ = make_row(emit.j, s, emit.r0, emit.r1, emit.r2, emit.r3);
        rows[v.row_base + qpos] = row_;
        TKAMD_PUBLISH_ROW(t, text, s, it.len, row_);
    }
}
// the first n_long workgroups (a multiple of three) take the three queues of longer words, a third of them each; the others the <= 16-byte queue
__global__ __launch_bounds__(256) void k_unigram_all(DevTables t, const uint8_t* __restrict__ text, QView v0, QView v1, QView v2, QView v3, uint4* __restrict__ rows,
                                                     uint32_t* __restrict__ tmp_ids, uint32_t* __restrict__ tmp_end, int* __restrict__ err, uint4* __restrict__ gstate,
                                                     uint32_t n_long) {
    __shared__ uint32_t s_qpre[NSQ + 1];
    __shared__ uint64_t s_best[UNI_LDS_POS];
    __shared__ uint32_t s_pk[UNI_LDS_POS];
    if (blockIdx.x >= n_long) {                               // (uniform per workgroup)
        unigram_body<0>(t, text, v0, rows, tmp_ids, tmp_end, err, gstate, blockIdx.x - n_long, gridDim.x - n_long, s_qpre, s_best, s_pk);
        return;
    }
    const uint32_t third = n_long / 3u, which = min(blockIdx.x / third, 2u);
    if (which == 0u) unigram_body<1>(t, text, v1, rows, tmp_ids, tmp_end, err, gstate, blockIdx.x, third, s_qpre, s_best, s_pk);
    else if (which == 1u) unigram_body<2>(t, text, v2, rows, tmp_ids, tmp_end, err, gstate, blockIdx.x - third, third, s_qpre, s_best, s_pk);
    else unigram_body<3>(t, text, v3, rows, tmp_ids, tmp_end, err, gstate, blockIdx.x - 2u * third, n_long - 2u * third, s_qpre, s_best, s_pk);
}

// =================================================================================================
// K_unigram_run_offsets: the offsets of byte-fallback tokens.  Every <0xXX> token of a run carries the offsets of the WHOLE run
// (unigram/model.rs:459: Token::new(id, byte_string, (offset, offset + len)) with the run's len -- "中é" as one run is five tokens, all
// (1, 3)).  k_token_meta gives every token the range of its own bytes snapped to its char -- right for a run of one char, the common
// case; a run of several chars is widened here, behind it: a lane per token, a fallback token takes the start of the first and the end
// of the last fallback token of its run.  Which tokens are fallback tokens, and where a run ends, is read off the result itself:
//   * a fallback token has the id of a <0xXX> piece and covers exactly ONE char (its own, snapped); the same id from the piece's
//     literal text "<0x41>" covers six.  In bytes: less than six (a char has at most four, the "▁" of a space one).
//   * two runs of one pre-token are never adjacent (the backtrack fuses them), a run never crosses a document, and the first char of a
//     pre-token that follows another in its document is a "▁", which is a piece (checked at load, host_model.cpp): no run starts there.
//     So neighbours that are both fallback tokens of one document are one run.
// Two launches: the first leaves a flag per token (from the offsets as k_token_meta wrote them), the second widens.  A lane reads the
// start of its run's first token and the end of its last, which the widening never changes.
// =================================================================================================
__global__ __launch_bounds__(256) void k_unigram_run_flags(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ offsets, const int64_t* __restrict__ n_tok,
                                                           const uint8_t* __restrict__ is_byte_id, uint32_t n_ids, uint8_t* __restrict__ flags) {
    const int64_t T = *n_tok;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
        const uint32_t id = ids[i];
        flags[i] = (id < n_ids && is_byte_id[id] && offsets[2 * i + 1] - offsets[2 * i] < 6u) ? 1 : 0;
    }
}
__global__ __launch_bounds__(256) void k_unigram_run_offsets(uint32_t* __restrict__ offsets, const int64_t* __restrict__ tok_offsets, int64_t n_docs,
                                                             const int64_t* __restrict__ n_tok, const uint8_t* __restrict__ flags) {
    const int64_t T = *n_tok;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
        if (!flags[i]) continue;
        if (!(i > 0 && flags[i - 1]) && !(i + 1 < T && flags[i + 1])) continue;      // (a run of one token, or of one char's: nothing to widen in most cases)
        // the document of token i: the last d with tok_offsets[d] <= i
        int64_t lo = 0, hi = n_docs;
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (tok_offsets[mid] <= i) lo = mid; else hi = mid; }
        const int64_t d0 = tok_offsets[lo], d1 = tok_offsets[lo + 1];
        int64_t a = i, b = i;
        while (a > d0 && flags[a - 1]) --a;
        while (b + 1 < d1 && flags[b + 1]) ++b;
        if (a != i) offsets[2 * i] = offsets[2 * a];
        if (b != i) offsets[2 * i + 1] = offsets[2 * b + 1];
    }
}
