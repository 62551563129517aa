// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers; it is not compiled on its own).  Decode_batch.

// =================================================================================================
// decode_batch: ids -> text.  Replaces Tokenizer::decode_batch / decode (tokenizer/mod.rs:1404-1416, 935-953) with the
// decoder folded into per-id byte strings at load time (host_model.cpp build_decode_tables): ByteLevel
// (pre_tokenizers/byte_level.rs:155-171), WordPiece (decoders/wordpiece.rs:46-64) and the no-decoder join.  A token
// contributes dec_blob[first-position form] if it is the first KEPT token of its sequence and the other form
// otherwise; unknown ids and (on request) special tokens contribute nothing.  Three passes: mark the first kept token
// of every sequence (only when some id has two forms), lengths + exclusive scan, gather.
// Round 5, for the BPE over characters round 4 added: BPEDecoder (decoders/bpe.rs:26-39: the end-of-word suffix becomes a space, and
// nothing on the LAST token -- the position with a form of its own is the last kept token then, `from_end`), Fuse (fuse.rs:24-29: the
// plain concatenation) and ByteFallback (byte_fallback.rs:27-67): a <0xXX> token is its byte, and a maximal run of such tokens that
// is not valid UTF-8 as a whole becomes one U+FFFD per byte -- k_decode_byte_runs walks every sequence once and marks those.
// =================================================================================================
// ---- the per-token rules, stated ONCE: the kernels of launch_decode (a lane a sequence for the masks, a lane a token for lengths and
// bytes) and the fused stream step (kernels/decode_stream.hip: a lane walks its own window) are written over these and nothing else ----
__device__ __forceinline__ bool dec_kept(uint32_t lenflags, uint32_t skip_special) {
    return !(lenflags & DEC_ABSENT) && !(skip_special && (lenflags & DEC_SPECIAL));
}
// is `id` a token the decoder sees (the id bound, then dec_kept)?  Its entry -> e.
__device__ __forceinline__ bool dec_kept_id(const uint4* __restrict__ entry, uint32_t n_ids, uint32_t skip_special, uint32_t id, uint4& e) {
    if (id >= n_ids) return false;                             // (no such token: dropped before the decoder sees the sequence)
    e = entry[id];
    return dec_kept(e.y, skip_special);
}
// the token of ids[b, end) with the position form of its own: the first kept one, or -- from_end (BPEDecoder) -- the last kept one; -1: none
__device__ __forceinline__ int64_t dec_form_token(const uint32_t* __restrict__ ids, int64_t b, int64_t end, const uint4* __restrict__ entry, uint32_t n_ids,
                                                  uint32_t skip_special, uint32_t from_end) {
    uint4 e;
    if (from_end) {
        for (int64_t t = end - 1; t >= b; --t)
            if (dec_kept_id(entry, n_ids, skip_special, ids[t], e)) return t;
        return -1;
    }
    for (int64_t t = b; t < end; ++t)
        if (dec_kept_id(entry, n_ids, skip_special, ids[t], e)) return t;
    return -1;
}
// ByteFallback::decode_chain (decoders/byte_fallback.rs:27-67): the KEPT tokens of a sequence in order; a maximal run of <0xXX> tokens is
// String::from_utf8 of its bytes, or -- if that fails -- one U+FFFD per byte.  A sequence is walked once: a run is validated
// as it goes (the UTF-8 automaton of the standard library: no overlong forms, no surrogates, nothing above U+10FFFF) and, if it fails,
// walked again to mark its tokens: mark(t) for every byte token of a failed run.
__device__ __forceinline__ bool utf8_step(uint32_t b, uint32_t& need, uint32_t& lo, uint32_t& hi) {      // false: invalid here
    if (need == 0u) {
        lo = 0x80u; hi = 0xBFu;
        if (b < 0x80u) return true;
        if (b >= 0xC2u && b <= 0xDFu) { need = 1u; return true; }
        if (b == 0xE0u) { need = 2u; lo = 0xA0u; return true; }
        if ((b >= 0xE1u && b <= 0xECu) || b == 0xEEu || b == 0xEFu) { need = 2u; return true; }
        if (b == 0xEDu) { need = 2u; hi = 0x9Fu; return true; }
        if (b == 0xF0u) { need = 3u; lo = 0x90u; return true; }
        if (b >= 0xF1u && b <= 0xF3u) { need = 3u; return true; }
        if (b == 0xF4u) { need = 3u; hi = 0x8Fu; return true; }
        return false;
    }
    if (b < lo || b > hi) return false;
    --need;
    lo = 0x80u; hi = 0xBFu;
    return true;
}
template <class Mark>
__device__ __forceinline__ void dec_bad_byte_runs(const uint32_t* __restrict__ ids, int64_t b, int64_t end, const uint4* __restrict__ entry, uint32_t n_ids,
                                                  uint32_t skip_special, Mark mark) {
    int64_t run0 = -1;                                         // first token of the run under way
    uint32_t need = 0u, lo = 0x80u, hi = 0xBFu;
    bool ok = true;
    auto close_run = [&](int64_t upto) {                       // the run [run0, upto) is over
        if (run0 >= 0 && (!ok || need != 0u))
            for (int64_t t = run0; t < upto; ++t) {
                uint4 e;
                if (dec_kept_id(entry, n_ids, skip_special, ids[t], e) && (e.y & DEC_BYTE)) mark(t);
            }
        run0 = -1; need = 0u; ok = true;
    };
    for (int64_t t = b; t < end; ++t) {
        uint4 e;
        if (!dec_kept_id(entry, n_ids, skip_special, ids[t], e)) continue;
        if (e.y & DEC_BYTE) {
            if (run0 < 0) run0 = t;
            if (ok) ok = utf8_step(e.x & 0xFFu, need, lo, hi);
        } else close_run(t);
    }
    close_run(end);
}
// CTC (decoders/ctc.rs:47-48: `.dedup()` over the kept tokens): a kept token whose id equals the kept id in front of it contributes
// nothing: mark(t) for every such token.
template <class Mark>
__device__ __forceinline__ void dec_dups(const uint32_t* __restrict__ ids, int64_t b, int64_t end, const uint4* __restrict__ entry, uint32_t n_ids,
                                         uint32_t skip_special, Mark mark) {
    uint32_t prev = 0xFFFFFFFFu;
    for (int64_t t = b; t < end; ++t) {
        const uint32_t id = ids[t];
        uint4 e;
        if (!dec_kept_id(entry, n_ids, skip_special, id, e)) continue;
        if (id == prev) mark(t);
        prev = id;
    }
}
// what a token that is kept and no duplicate contributes.  A byte token: U+FFFD -- three bytes -- if its run is not UTF-8, else its byte
// (as the first kept token under a leading Strip of that very byte the first-position form has length 0); any other: its string in
// the form of its position.
__device__ __forceinline__ uint32_t dec_piece_len(const uint4& e, bool first, bool bad) {
    if ((e.y & DEC_BYTE) && bad) return 3u;
    return first ? (e.y & DEC_LEN_MASK) : e.w;
}
__device__ __forceinline__ void dec_piece_write(const uint4& e, bool first, bool bad, const uint8_t* __restrict__ blob, uint8_t* __restrict__ dst) {
    if (e.y & DEC_BYTE) {
        if (bad) { dst[0] = 0xEFu; dst[1] = 0xBFu; dst[2] = 0xBDu; }
        else if ((first ? (e.y & DEC_LEN_MASK) : e.w) != 0u) dst[0] = (uint8_t)e.x;
        return;
    }
    const uint32_t off = first ? e.x : e.z, l = first ? (e.y & DEC_LEN_MASK) : e.w;
    const uint8_t* src = blob + off;
    for (uint32_t i = 0; i < l; ++i) dst[i] = src[i];
}
__device__ __forceinline__ bool dec_mask_bit(const uint32_t* __restrict__ mask, int64_t t) { return mask && ((mask[t >> 5] >> (t & 31)) & 1u); }

__global__ __launch_bounds__(256) void k_decode_first(const uint32_t* __restrict__ ids, const int64_t* __restrict__ tok_off, int64_t n_docs,
                                                      const uint4* __restrict__ entry, uint32_t n_ids, uint32_t skip_special,
                                                      uint32_t* __restrict__ firstmask, uint32_t from_end) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_docs) return;
    const int64_t t = dec_form_token(ids, tok_off[d], tok_off[d + 1], entry, n_ids, skip_special, from_end);
    if (t >= 0) atomicOr(&firstmask[t >> 5], 1u << (t & 31));
}
// one lane per sequence
__global__ __launch_bounds__(256) void k_decode_byte_runs(const uint32_t* __restrict__ ids, const int64_t* __restrict__ tok_off, int64_t n_docs,
                                                          const uint4* __restrict__ entry, uint32_t n_ids, uint32_t skip_special,
                                                          uint32_t* __restrict__ badmask) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_docs) return;
    dec_bad_byte_runs(ids, tok_off[d], tok_off[d + 1], entry, n_ids, skip_special, [&](int64_t t) { atomicOr(&badmask[t >> 5], 1u << (t & 31)); });
}
// one lane per sequence
__global__ __launch_bounds__(256) void k_decode_dups(const uint32_t* __restrict__ ids, const int64_t* __restrict__ tok_off, int64_t n_docs,
                                                     const uint4* __restrict__ entry, uint32_t n_ids, uint32_t skip_special, uint32_t* __restrict__ dupmask) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_docs) return;
    dec_dups(ids, tok_off[d], tok_off[d + 1], entry, n_ids, skip_special, [&](int64_t t) { atomicOr(&dupmask[t >> 5], 1u << (t & 31)); });
}
__global__ __launch_bounds__(256) void k_decode_len(const uint32_t* __restrict__ ids, int64_t n_tok, const uint4* __restrict__ entry, uint32_t n_ids,
                                                    uint32_t skip_special, const uint32_t* __restrict__ firstmask, const uint32_t* __restrict__ badmask,
                                                    const uint32_t* __restrict__ dupmask, uint32_t* __restrict__ len) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    uint4 e;
    uint32_t l = 0;
    if (dec_kept_id(entry, n_ids, skip_special, ids[t], e) && !dec_mask_bit(dupmask, t)) l = dec_piece_len(e, dec_mask_bit(firstmask, t), dec_mask_bit(badmask, t));
    len[t] = l;
}
__global__ __launch_bounds__(256) void k_decode_doc_off(const int64_t* __restrict__ tok_off, int64_t n_docs, const uint32_t* __restrict__ pos,
                                                        int64_t n_tok, const int64_t* __restrict__ total, int64_t* __restrict__ out_off) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d > n_docs) return;
    const int64_t t = tok_off[d];
    out_off[d] = t < n_tok ? (int64_t)pos[t] : *total;
}
__global__ __launch_bounds__(256) void k_decode_copy(const uint32_t* __restrict__ ids, int64_t n_tok, const uint4* __restrict__ entry, uint32_t n_ids,
                                                     uint32_t skip_special, const uint32_t* __restrict__ firstmask, const uint32_t* __restrict__ badmask,
                                                     const uint32_t* __restrict__ dupmask, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ pos,
                                                     uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    uint4 e;
    if (!dec_kept_id(entry, n_ids, skip_special, ids[t], e) || dec_mask_bit(dupmask, t)) return;
    dec_piece_write(e, dec_mask_bit(firstmask, t), dec_mask_bit(badmask, t), blob, out + pos[t]);
}
// ONE lane decodes ONE short sequence ids[0, k) into dst (the fused stream step: a window is a few ids): the passes of launch_decode in
// their order -- the position form, the byte runs, the dedup, then lengths and bytes token by token -- with the three masks as bits of
// flag[0, k), a byte a token in the lane's own scratch.  Returns the bytes written: at most k x the longest per-id string (3 for a
// byte token of a failed run).
struct DecSeqView {
    const uint4* entry;
    const uint8_t* blob;
    uint32_t n_ids, skip_special;
    uint32_t position_forms, from_end, byte_runs, dedup;       // which masks launch_decode would be given (HostModel dec_*)
};
constexpr uint8_t DEC_F_FORM = 1, DEC_F_BAD = 2, DEC_F_DUP = 4;
__device__ __forceinline__ uint32_t dec_lane_sequence(const DecSeqView& v, const uint32_t* __restrict__ ids, uint32_t k, uint8_t* __restrict__ flag,
                                                      uint8_t* __restrict__ dst) {
    for (uint32_t t = 0; t < k; ++t) flag[t] = 0;
    if (v.position_forms) {
        const int64_t t = dec_form_token(ids, 0, (int64_t)k, v.entry, v.n_ids, v.skip_special, v.from_end);
        if (t >= 0) flag[t] |= DEC_F_FORM;
    }
    if (v.byte_runs) dec_bad_byte_runs(ids, 0, (int64_t)k, v.entry, v.n_ids, v.skip_special, [&](int64_t t) { flag[t] |= DEC_F_BAD; });
    if (v.dedup) dec_dups(ids, 0, (int64_t)k, v.entry, v.n_ids, v.skip_special, [&](int64_t t) { flag[t] |= DEC_F_DUP; });
    uint32_t at = 0u;
    for (uint32_t t = 0; t < k; ++t) {
        uint4 e;
        const uint8_t f = flag[t];
        if (!dec_kept_id(v.entry, v.n_ids, v.skip_special, ids[t], e) || (f & DEC_F_DUP)) continue;
        dec_piece_write(e, (f & DEC_F_FORM) != 0, (f & DEC_F_BAD) != 0, v.blob, dst + at);
        at += dec_piece_len(e, (f & DEC_F_FORM) != 0, (f & DEC_F_BAD) != 0);
    }
    return at;
}
// what a byte that contributes l bytes (utf8_lossy_len) leaves at dst: itself, U+FFFD, or nothing
__device__ __forceinline__ void lossy_put(uint32_t l, uint8_t b, uint8_t* __restrict__ dst) {
    if (l == 1u) dst[0] = b;
    else if (l == 3u) { dst[0] = 0xEFu; dst[1] = 0xBFu; dst[2] = 0xBDu; }
}
// String::from_utf8_lossy of ONE sequence src[0, n) by one lane, the sequence's own bounds as utf8_lossy_len's: dst gets the repaired
// text, at most 3 bytes a source byte.  Returns its length.
__device__ __forceinline__ uint32_t lossy_lane_sequence(const uint8_t* __restrict__ src, uint32_t n, uint8_t* __restrict__ dst) {
    uint32_t at = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = utf8_lossy_len(src, (int64_t)i, 0, (int64_t)n);
        lossy_put(l, src[i], dst + at);
        at += l;
    }
    return at;
}
void launch_decode(hipStream_t st, const uint32_t* ids, const int64_t* tok_off, int64_t n_docs, int64_t n_tok, const void* entry, uint32_t n_ids,
                   const uint8_t* blob, uint32_t skip_special, uint32_t* firstmask, uint32_t* len, uint32_t* bsum, uint32_t* pos, int64_t* total,
                   int64_t* out_off, uint8_t* out_bytes_or_null, uint32_t from_end, uint32_t* badmask, uint32_t* dupmask) {
    const uint4* e = (const uint4*)entry;
    if (!out_bytes_or_null) {                                 // phase 1: lengths, positions, document offsets, total
        (void)hipMemsetAsync(total, 0, 8, st);
        if (n_tok > 0) {
            if (firstmask && n_docs > 0) {
                (void)hipMemsetAsync(firstmask, 0, (size_t)((n_tok >> 5) + 1) * 4, st);
                hipLaunchKernelGGL(k_decode_first, dim3(blocks_for(n_docs, 256)), dim3(256), 0, st, ids, tok_off, n_docs, e, n_ids, skip_special, firstmask, from_end);
            }
            if (badmask && n_docs > 0) {
                (void)hipMemsetAsync(badmask, 0, (size_t)((n_tok >> 5) + 1) * 4, st);
                hipLaunchKernelGGL(k_decode_byte_runs, dim3(blocks_for(n_docs, 256)), dim3(256), 0, st, ids, tok_off, n_docs, e, n_ids, skip_special, badmask);
            }
            if (dupmask && n_docs > 0) {
                (void)hipMemsetAsync(dupmask, 0, (size_t)((n_tok >> 5) + 1) * 4, st);
                hipLaunchKernelGGL(k_decode_dups, dim3(blocks_for(n_docs, 256)), dim3(256), 0, st, ids, tok_off, n_docs, e, n_ids, skip_special, dupmask);
            }
            const unsigned nb = blocks_for(n_tok, 256);
            hipLaunchKernelGGL(k_decode_len, dim3(nb), dim3(256), 0, st, ids, n_tok, e, n_ids, skip_special, (const uint32_t*)firstmask, (const uint32_t*)badmask,
                               (const uint32_t*)dupmask, len);
            hipLaunchKernelGGL(k_u32_reduce, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, n_tok, bsum);
            hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, bsum, (int64_t)nb, (const int64_t*)nullptr, (int64_t)1, total);
            hipLaunchKernelGGL(k_u32_down, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, n_tok, (const uint32_t*)bsum, pos);
        }
        hipLaunchKernelGGL(k_decode_doc_off, dim3(blocks_for(n_docs + 1, 256)), dim3(256), 0, st, tok_off, n_docs, (const uint32_t*)pos, n_tok,
                           (const int64_t*)total, out_off);
    } else if (n_tok > 0) {                                   // phase 2: gather (the caller sized out_bytes from *total)
        hipLaunchKernelGGL(k_decode_copy, dim3(blocks_for(n_tok, 256)), dim3(256), 0, st, ids, n_tok, e, n_ids, skip_special,
                           (const uint32_t*)firstmask, (const uint32_t*)badmask, (const uint32_t*)dupmask, blob, (const uint32_t*)pos, out_bytes_or_null);
    }
}

// =================================================================================================
// The device entry of decode_batch (tkamd_decode_batch_device): the ids are in HBM already, as any int32 / uint32 / int64 array and one
// [begin, end) range per sequence -- a packed CSR, the rows of a padded [B, L] tensor, ranges in any order --, and the text stays
// there.  Two pieces in front of and behind launch_decode, which runs unchanged between them:
//   the range gather  lengths of the ranges (a range that is not inside [0, n_elems] counts nothing and is reported), their scan into
//                     the token CSR launch_decode reads, and the ids copied -- one lane per id -- into the contiguous uint32 array;
//   the lossy repair  String::from_utf8_lossy per sequence (the ByteLevel decoder only: every other decoder emits token strings, and
//                     ByteFallback's badmask writes U+FFFD itself): utf8_lossy_core.hpp decides per byte, k_lossy_count sums what the
//                     repaired text would hold and how many invalid subparts there are in one pass over the text, and only a text
//                     that has one pays for the length pass, the scan and the scatter.
// scalars (int64[8], dw_total): [0] bytes of the text (launch_decode), [1] tokens as the u32 scan has them, [2] the first bad range as
// (n_docs - d) << 4 | why (0: none), [3] tokens summed in 64 bits (what the host's limit is held against), [4] bytes of the repaired text, [5] invalid subparts.
// =================================================================================================
constexpr int DECS_N_TOK = 1, DECS_BAD = 2, DECS_N_TOK64 = 3, DECS_FIXED = 4, DECS_INVALID = 5;

// the last index d in [0, n] with off[d] <= x (off ascending, off[0] <= x)
template <class T>
__device__ __forceinline__ int64_t dec_owner(const T* __restrict__ off, int64_t n, uint64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((uint64_t)off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__global__ __launch_bounds__(256) void k_decode_range_len(const int64_t* __restrict__ begin, const int64_t* __restrict__ end, int64_t n_docs, int64_t n_elems,
                                                          uint32_t* __restrict__ len, unsigned long long* __restrict__ scalars) {
    __shared__ uint32_t sm[4];
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t l = 0u;
    if (d < n_docs) {
        const int64_t b = begin[d], e = end[d];
        const uint32_t why = (b > e ? 1u : 0u) | (b < 0 ? 2u : 0u) | (e > n_elems ? 4u : 0u);
        if (why) atomicMax(&scalars[DECS_BAD], ((unsigned long long)(n_docs - d) << 4) | why);
        else if (e - b >= ((int64_t)1 << 31)) atomicMax(&scalars[DECS_BAD], ((unsigned long long)(n_docs - d) << 4) | 8u);
        else l = (uint32_t)(e - b);
    }
    if (d <= n_docs) len[d] = l;                               // (len[n_docs] = 0: its position is the token count)
    // the token count in 64 bits, next to the u32 scan: ranges may overlap, so their lengths can sum past 2^32 over a small array and the
    // scan's total would wrap under the host's limit.  Two 16-bit halves through the u32 block sum (256 x 65,535 fits), one add a workgroup.
    uint32_t t_lo, t_hi;
    block256_excl_scan(l & 0xFFFFu, sm, &t_lo);
    block256_excl_scan(l >> 16, sm, &t_hi);
    if (threadIdx.x == 0 && (t_lo | t_hi)) atomicAdd(&scalars[DECS_N_TOK64], ((unsigned long long)t_hi << 16) + t_lo);
}
__global__ __launch_bounds__(256) void k_decode_tok_off(const uint32_t* __restrict__ pos, int64_t n_docs, int64_t* __restrict__ tok_off) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d <= n_docs) tok_off[d] = (int64_t)pos[d];
}
// one lane per id: the sequence it belongs to is the last one that starts at or before it (empty ones in between start where it does
// not: they are skipped by taking the LAST), its source the same distance into that sequence's range.  WIDE: the ids are int64; a
// value that is no uint32 becomes 0xFFFFFFFF, an id no vocabulary has.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_decode_gather(const void* __restrict__ src, const int64_t* __restrict__ begin, const uint32_t* __restrict__ pos,
                                                       int64_t n_docs, int64_t n_tok, uint32_t* __restrict__ ids) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    const int64_t d = dec_owner(pos, n_docs, (uint64_t)t);     // (pos[n_docs] = n_tok > t: d < n_docs)
    const int64_t s = begin[d] + (t - (int64_t)pos[d]);
    if (WIDE) {
        const int64_t v = ((const int64_t*)src)[s];
        ids[t] = (v < 0 || v > (int64_t)0xFFFFFFFFll) ? 0xFFFFFFFFu : (uint32_t)v;
    } else ids[t] = ((const uint32_t*)src)[s];
}
void launch_decode_ranges(hipStream_t st, const int64_t* begin, const int64_t* end, int64_t n_docs, int64_t n_elems, uint32_t* len, uint32_t* bsum,
                          uint32_t* pos, int64_t* tok_off, int64_t* scalars) {
    (void)hipMemsetAsync(scalars + 1, 0, 7 * 8, st);
    const unsigned nb = blocks_for(n_docs + 1, 256);
    hipLaunchKernelGGL(k_decode_range_len, dim3(nb), dim3(256), 0, st, begin, end, n_docs, n_elems, len, (unsigned long long*)scalars);
    hipLaunchKernelGGL(k_u32_reduce, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, n_docs + 1, bsum);
    hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, bsum, (int64_t)nb, (const int64_t*)nullptr, (int64_t)1, scalars + DECS_N_TOK);
    hipLaunchKernelGGL(k_u32_down, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, n_docs + 1, (const uint32_t*)bsum, pos);
    hipLaunchKernelGGL(k_decode_tok_off, dim3(nb), dim3(256), 0, st, (const uint32_t*)pos, n_docs, tok_off);
}
void launch_decode_gather(hipStream_t st, const void* src, bool wide, const int64_t* begin, const uint32_t* pos, int64_t n_docs, int64_t n_tok, uint32_t* ids) {
    if (n_tok <= 0) return;
    const unsigned nb = blocks_for(n_tok, 256);
    if (wide) hipLaunchKernelGGL(k_decode_gather<true>, dim3(nb), dim3(256), 0, st, src, begin, pos, n_docs, n_tok, ids);
    else hipLaunchKernelGGL(k_decode_gather<false>, dim3(nb), dim3(256), 0, st, src, begin, pos, n_docs, n_tok, ids);
}

// the sequence byte i lies in: [lo, hi) from the text's document CSR
__device__ __forceinline__ void lossy_bounds(const int64_t* __restrict__ doc_off, int64_t n_docs, int64_t i, int64_t& lo, int64_t& hi) {
    const int64_t d = dec_owner(doc_off, n_docs, (uint64_t)i); // (doc_off[n_docs] = n > i: d < n_docs)
    lo = doc_off[d];
    hi = doc_off[d + 1];
}
// 16 bytes a lane, one 16-byte load; a lane whose bytes are all ASCII -- nearly every lane of nearly every text -- is done with that
__global__ __launch_bounds__(256) void k_lossy_count(const uint8_t* __restrict__ text, int64_t n, const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                     unsigned long long* __restrict__ scalars) {
    __shared__ uint32_t sm[4];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    uint32_t extra = 0u, gone = 0u, invalid = 0u;             // bytes the repair adds / drops, invalid subparts
    if (i0 < n) {
        const uint4 w = *(const uint4*)(text + i0);           // (the buffer is 16-byte aligned and has TEXT_PAD bytes behind n)
        if ((w.x | w.y | w.z | w.w) & 0x80808080u) {
            const int64_t i1 = min(i0 + 16, n);
            int64_t lo = 0, hi = -1;
            for (int64_t i = i0; i < i1; ++i) {
                if (text[i] < 0x80u) continue;
                if (i >= hi) lossy_bounds(doc_off, n_docs, i, lo, hi);
                const uint32_t l = utf8_lossy_len(text, i, lo, hi);
                if (l == 3u) { extra += 2u; ++invalid; }
                else if (l == 0u) ++gone;
            }
        }
    }
    // (three block sums through the one scan helper: they are off the common path's cost -- a launch over the text at 16 bytes a lane)
    uint32_t t_extra, t_gone, t_invalid;
    block256_excl_scan(extra, sm, &t_extra);
    block256_excl_scan(gone, sm, &t_gone);
    block256_excl_scan(invalid, sm, &t_invalid);
    if (threadIdx.x == 0) {
        const int64_t i1 = min((int64_t)(blockIdx.x + 1) * 4096, n);
        atomicAdd(&scalars[DECS_FIXED], (unsigned long long)(i1 - (int64_t)blockIdx.x * 4096) + t_extra - t_gone);
        if (t_invalid) atomicAdd(&scalars[DECS_INVALID], (unsigned long long)t_invalid);
    }
}
__global__ __launch_bounds__(256) void k_lossy_len(const uint8_t* __restrict__ text, int64_t n, const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                   uint32_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t l = 1u;
    if (text[i] >= 0x80u) {
        int64_t lo, hi;
        lossy_bounds(doc_off, n_docs, i, lo, hi);
        l = utf8_lossy_len(text, i, lo, hi);
    }
    len[i] = l;
}
__global__ __launch_bounds__(256) void k_lossy_scatter(const uint8_t* __restrict__ text, int64_t n, const uint32_t* __restrict__ len, const uint32_t* __restrict__ pos,
                                                       uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    lossy_put(len[i], text[i], out + pos[i]);
}
// the document CSR follows its text: in place, a lane an entry
__global__ __launch_bounds__(256) void k_lossy_doc_off(int64_t* __restrict__ doc_off, int64_t n_docs, const uint32_t* __restrict__ pos, int64_t n,
                                                       const int64_t* __restrict__ total) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d > n_docs) return;
    const int64_t o = doc_off[d];
    doc_off[d] = o < n ? (int64_t)pos[o] : *total;
}
void launch_utf8_lossy_count(hipStream_t st, const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs, int64_t* scalars) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_lossy_count, dim3(blocks_for((n + 15) / 16, 256)), dim3(256), 0, st, text, n, doc_off, n_docs, (unsigned long long*)scalars);
}
void launch_utf8_lossy_repair(hipStream_t st, const uint8_t* text, int64_t n, int64_t* doc_off, int64_t n_docs, uint32_t* len, uint32_t* bsum, uint32_t* pos,
                              int64_t* total, uint8_t* out) {
    if (n <= 0) return;
    const unsigned nb = blocks_for(n, 256);
    hipLaunchKernelGGL(k_lossy_len, dim3(nb), dim3(256), 0, st, text, n, (const int64_t*)doc_off, n_docs, len);
    hipLaunchKernelGGL(k_u32_reduce, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, n, bsum);
    hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, bsum, (int64_t)nb, (const int64_t*)nullptr, (int64_t)1, total);
    hipLaunchKernelGGL(k_u32_down, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, n, (const uint32_t*)bsum, pos);
    hipLaunchKernelGGL(k_lossy_scatter, dim3(nb), dim3(256), 0, st, text, n, (const uint32_t*)len, (const uint32_t*)pos, out);
    hipLaunchKernelGGL(k_lossy_doc_off, dim3(blocks_for(n_docs + 1, 256)), dim3(256), 0, st, doc_off, n_docs, (const uint32_t*)pos, n, (const int64_t*)total);
}
// the TEXT_PAD readable zero bytes an encode over this text expects behind it
void launch_decode_zero_pad(hipStream_t st, uint8_t* text, const int64_t* n_dev) {
    hipLaunchKernelGGL(k_zero_tail, dim3(1), dim3(64), 0, st, text, n_dev, (int)TEXT_PAD, (unsigned long long*)nullptr, (int64_t)0);
}
