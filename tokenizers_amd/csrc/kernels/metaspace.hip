// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers and kernels/bert_norm.hip, whose SWAR helpers and output-size layout it shares; it is not compiled on its own).
// The "▁" front of SentencePiece-style BPE.

// =================================================================================================
// The X text of the "▁" front: every ' ' of a piece becomes "▁" (U+2581, E2 96 81: normalizers/replace.rs:83, or Metaspace's own replace,
// pre_tokenizers/metaspace.rs:122-146), and a piece -- what lies between document edges and added-token matches -- that takes a prepend
// under the scheme (tables.hpp MsPrepend) gets one "▁" in front, aligned to its first char (tokenizer/normalizer.rs:503-514).  The bytes
// of added-token matches are copied as they are.  The shape is the BertNormalizer's (kernels/bert_norm.hip): k_ms_count sizes the output
// of every source byte (one byte per 16-byte lane, the per-byte array only where a lane is not plain -- BnOlen), the scan places the
// 64-byte words, k_ms_write writes the X text and, with offsets, the original byte of every X byte (the start of its source char: the end
// follows from it, kernels/output.hip norig_end).  Then k_ms_units marks the pre-tokens in X: every piece start, and every "▁" behind a
// char other than "▁" (Metaspace split = false / no pre-tokenizer: the units the load-time merge check proves exact) or every "▁" at all
// (split = true: MergedWithNext, the reference's own pre-tokens).
// =================================================================================================
struct MsArgs {
    const uint8_t* text;
    int64_t n_bytes;
    const unsigned long long* pstart;     // piece starts over the raw text: documents + match edges
    const unsigned long long* dstart;     // document starts over the raw text (MS_FIRST)
    const unsigned long long* mmask;      // added-token matches: first bytes, and the bytes inside them (null: no matches)
    const unsigned long long* smask;
    uint32_t prepend;                     // MsPrepend
    const int64_t* len_dev;               // behind a normalizer: the text is its output, *len_dev bytes of the n_bytes the host bounds it by (null: n_bytes)
    const uint32_t* map;                  // ... and this is the original byte of every byte of it: the source map is composed with it (null: the raw text)
};

__device__ __forceinline__ bool ms_bit(const unsigned long long* __restrict__ m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; }
__device__ __forceinline__ bool ms_is_bar(const uint8_t* __restrict__ p) { return p[0] == 0xE2u && p[1] == 0x96u && p[2] == 0x81u; }

// char::is_whitespace (the White_Space property) as UTF-8: the length of the whitespace char that starts at p, or 0
__device__ __forceinline__ uint32_t ms_ws_len(const uint8_t* __restrict__ p) {
    const uint32_t b = p[0];
    if (b < 0x80u) return (b == 0x20u || b - 9u < 5u) ? 1u : 0u;
    if (b == 0xC2u) return (p[1] == 0x85u || p[1] == 0xA0u) ? 2u : 0u;
    if (b == 0xE1u) return (p[1] == 0x9Au && p[2] == 0x80u) ? 3u : 0u;
    if (b == 0xE2u) return ((p[1] == 0x80u && (p[2] - 0x80u < 11u || p[2] == 0xA8u || p[2] == 0xA9u || p[2] == 0xAFu)) || (p[1] == 0x81u && p[2] == 0x9Fu)) ? 3u : 0u;
    if (b == 0xE3u) return (p[1] == 0x80u && p[2] == 0x80u) ? 3u : 0u;
    return 0u;
}
// is byte i (i > 0) behind a whitespace char
__device__ __forceinline__ bool ms_behind_ws(const uint8_t* __restrict__ text, int64_t i) {
    const uint32_t b = text[i - 1];
    if (b < 0x80u) return b == 0x20u || b - 9u < 5u;
    return (i >= 2 && ms_ws_len(text + i - 2) == 2u) || (i >= 3 && ms_ws_len(text + i - 3) == 3u);
}
// MS_WORD (Sequence[WhitespaceSplit, Metaspace "always"]): whitespace chars are dropped; the first char of a word -- behind whitespace, or
// at a piece start -- takes a "▁" in front unless it is one
__device__ __forceinline__ uint32_t ms_word_count(const MsArgs& a, int64_t i, uint32_t b, bool piece_start) {
    if ((b & 0xC0u) == 0x80u) {                                       // a continuation byte: nothing if its char is whitespace
        for (int k = 1; k <= 2 && i - k >= 0; ++k) {
            const uint32_t c = a.text[i - k];
            if ((c & 0xC0u) == 0x80u) continue;
            return ms_ws_len(a.text + i - k) > (uint32_t)k ? 0u : 1u;
        }
        return 1u;
    }
    if (ms_ws_len(a.text + i)) return 0u;
    return 1u + (((piece_start || ms_behind_ws(a.text, i)) && !ms_is_bar(a.text + i)) ? 3u : 0u);
}

// does the piece that starts at source byte i (b = text[i]) take a "▁" in front
__device__ __forceinline__ bool ms_takes_prepend(const MsArgs& a, int64_t i, uint32_t b) {
    if (a.prepend == MS_PIECE) return true;
    if (a.prepend == MS_NEVER) return false;
    if (a.prepend == MS_FIRST && !ms_bit(a.dstart, i)) return false;      // offsets_original().0 != 0: behind an added token
    return !(b == 0x20u || ms_is_bar(a.text + i));                       // (after the replace it starts with "▁" already)
}

// output bytes of source byte i, the per-byte way
__device__ __forceinline__ uint32_t ms_count_byte(const MsArgs& a, int64_t i, uint32_t b, bool verbatim, bool piece_start) {
    if (verbatim) return 1u;
    if (a.prepend == MS_WORD) return ms_word_count(a, i, b, piece_start);
    return (b == 0x20u ? 3u : 1u) + ((piece_start && ms_takes_prepend(a, i, b)) ? 3u : 0u);
}

__global__ __launch_bounds__(256) void k_ms_count(MsArgs a, uint8_t* __restrict__ olen, uint8_t* __restrict__ ltot, uint32_t* __restrict__ wsum) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * BN_LANE;
    const int64_t n = a.len_dev ? *a.len_dev : a.n_bytes;         // (lanes between the text's end and its bound leave zeros: the scan covers the bound)
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    bool plain = false;                                             // sixteen ASCII bytes, no space, no piece start, no match: one output byte each
    if (i0 < n) {
        const Unaligned16 t = *(const Unaligned16*)(a.text + i0);   // (readable TEXT_PAD bytes past the end)
        const uint32_t x[4] = {t.a, t.b, t.c, t.d};
        const uint32_t vb = a.mmask ? (mask16(a.mmask, i0) | mask16(a.smask, i0)) : 0u;
        const uint32_t pb = mask16(a.pstart, i0);
        uint32_t sp = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) sp |= a.prepend == MS_WORD ? sw_lt(x[k], 0x21u) : sw_eq(x[k], 0x20u);
        // (MS_WORD: no whitespace in the lane, and an ASCII char that is none in front of it -- else the first byte may open a word)
        if (a.prepend == MS_WORD && i0 > 0 && a.text[i0 - 1] - 0x21u >= 0x5Fu) sp = 1u;
        if (((t.a | t.b | t.c | t.d) & SW_H) == 0u && sp == 0u && (vb | pb) == 0u && i0 + BN_LANE <= n) {
            plain = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = SW_1;
        } else {
            const int nv = (int)min((int64_t)BN_LANE, n - i0);
            for (int j = 0; j < nv; ++j)
                o[j >> 2] |= ms_count_byte(a, i0 + j, (x[j >> 2] >> (8 * (j & 3))) & 0xFFu, (vb >> j) & 1u, (pb >> j) & 1u) << (8 * (j & 3));
            *(uint4*)(olen + i0) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    uint32_t s = ((o[0] * SW_1) >> 24) + ((o[1] * SW_1) >> 24) + ((o[2] * SW_1) >> 24) + ((o[3] * SW_1) >> 24);     // (<= 96: six bytes a source byte)
    if (i0 < a.n_bytes) ltot[i0 >> 4] = (uint8_t)(s | (plain ? BN_LTOT_PLAIN : 0u));
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if ((threadIdx.x & 3) == 0 && i0 <= a.n_bytes) wsum[i0 >> 6] = s;
}

__global__ __launch_bounds__(256) void k_ms_write(MsArgs a, BnOlen olen, const uint32_t* __restrict__ wbase, uint8_t* __restrict__ xtext, uint32_t* __restrict__ nos) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * BN_LANE;
    const uint32_t lt = i0 < a.n_bytes ? (uint32_t)olen.ltot[i0 >> 4] : 0u;
    const uint32_t tot = lt & 0x7Fu;
    const int lane = lane_id();
    const uint32_t t1 = (uint32_t)__shfl_up((int)tot, 1, 64), t2 = (uint32_t)__shfl_up((int)tot, 2, 64), t3 = (uint32_t)__shfl_up((int)tot, 3, 64);
    const int sub = lane & 3;
    if (!tot) return;
    uint32_t pos = wbase[i0 >> 6] + (sub >= 1 ? t1 : 0u) + (sub >= 2 ? t2 : 0u) + (sub >= 3 ? t3 : 0u);
    const Unaligned16 t = *(const Unaligned16*)(a.text + i0);
    if (lt & BN_LTOT_PLAIN) {
        *(Unaligned16*)(xtext + pos) = t;
        if (nos && a.map) {
#pragma unroll
            for (int j = 0; j < BN_LANE; j += 4) *(Unaligned16*)(nos + pos + j) = *(const Unaligned16*)(a.map + i0 + j);
        } else if (nos) {
            const uint32_t b0 = (uint32_t)i0;
#pragma unroll
            for (int j = 0; j < BN_LANE; j += 4) *(Unaligned16*)(nos + pos + j) = Unaligned16{b0 + j, b0 + j + 1u, b0 + j + 2u, b0 + j + 3u};
        }
        return;
    }
    const int64_t n = a.len_dev ? *a.len_dev : a.n_bytes;
    const uint32_t x[4] = {t.a, t.b, t.c, t.d};
    const uint32_t vb = a.mmask ? (mask16(a.mmask, i0) | mask16(a.smask, i0)) : 0u;
    const uint32_t pb = mask16(a.pstart, i0);
    const int nv = (int)min((int64_t)BN_LANE, n - i0);
    for (int j = 0; j < nv; ++j) {
        const int64_t i = i0 + j;
        const uint32_t b = (x[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        if ((vb >> j) & 1u) {                                       // a match byte: verbatim, its own original byte
            xtext[pos] = (uint8_t)b;
            if (nos) nos[pos] = a.map ? a.map[i] : (uint32_t)i;
            ++pos;
            continue;
        }
        if (a.prepend == MS_WORD) {                                 // whitespace dropped, a "▁" in front of a word's first char
            const uint32_t c = ms_word_count(a, i, b, (pb >> j) & 1u);
            if (!c) continue;
            uint32_t cs = (uint32_t)i;
            if (nos) {
                if ((b & 0xC0u) == 0x80u) { int k = 0; while (k < 3 && cs > 0u && (a.text[cs] & 0xC0u) == 0x80u) { --cs; ++k; } }
                if (a.map) cs = a.map[cs];
            }
            if (c > 1u) {
                xtext[pos] = 0xE2u; xtext[pos + 1] = 0x96u; xtext[pos + 2] = 0x81u;
                if (nos) { nos[pos] = cs; nos[pos + 1] = cs; nos[pos + 2] = cs; }
                pos += 3;
            }
            xtext[pos] = (uint8_t)b;
            if (nos) nos[pos] = cs;
            ++pos;
            continue;
        }
        // the start of the source char (a continuation byte belongs to the char in front of it: its alignment is that char's whole range)
        uint32_t cs = (uint32_t)i;
        if (nos && (b & 0xC0u) == 0x80u) { int k = 0; while (k < 3 && cs > 0u && (a.text[cs] & 0xC0u) == 0x80u) { --cs; ++k; } }
        const uint32_t ci = (nos && a.map) ? a.map[i] : (uint32_t)i;
        if (nos && a.map) cs = a.map[cs];
        if (((pb >> j) & 1u) && ms_takes_prepend(a, i, b)) {
            xtext[pos] = 0xE2u; xtext[pos + 1] = 0x96u; xtext[pos + 2] = 0x81u;
            if (nos) { nos[pos] = cs; nos[pos + 1] = cs; nos[pos + 2] = cs; }
            pos += 3;
        }
        if (b == 0x20u) {
            xtext[pos] = 0xE2u; xtext[pos + 1] = 0x96u; xtext[pos + 2] = 0x81u;
            if (nos) { nos[pos] = ci; nos[pos + 1] = ci; nos[pos + 2] = ci; }
            pos += 3;
        } else {
            xtext[pos] = (uint8_t)b;
            if (nos) nos[pos] = cs;
            ++pos;
        }
    }
}

// bit k (k < 4): byte k of w equals c
__device__ __forceinline__ uint32_t ms_eq4(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);       // 0x80 exactly where a byte of x is zero
    return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
}
// bits of the 64 bytes at p (64-byte aligned in the text) that equal c
__device__ __forceinline__ unsigned long long ms_eq64(const uint4* __restrict__ p4, uint32_t c) {
    unsigned long long m = 0ull;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = p4[q];
        const uint32_t bits = ms_eq4(v.x, c) | (ms_eq4(v.y, c) << 4) | (ms_eq4(v.z, c) << 8) | (ms_eq4(v.w, c) << 12);
        m |= (unsigned long long)bits << (16 * q);
    }
    return m;
}

// Pre-token starts of the X text: a lane per 64-byte word.  bars = the first bytes of "▁" (E2 96 81 -- in UTF-8 that sequence is the char
// and nothing else); behind a char other than "▁" unless split; every piece start (pmask: documents + match edges in X); nothing at or
// beyond the text's length.  (k_apply_matches then makes every match one pre-token.)
__global__ __launch_bounds__(256) void k_ms_units(const uint8_t* __restrict__ x, int64_t n_host, const int64_t* __restrict__ len_dev,
                                                  const unsigned long long* __restrict__ pmask, unsigned long long* __restrict__ startmask, int64_t n_words, uint32_t split) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    const int64_t n = len_dev ? *len_dev : n_host;
    const int64_t b0 = w << 6;
    if (b0 >= n) { startmask[w] = 0ull; return; }
    // (the X text is a workspace buffer: 16-byte aligned, readable TEXT_PAD bytes past its end, zero there)
    const uint4* p4 = (const uint4*)(x + b0);
    const unsigned long long e2 = ms_eq64(p4, 0xE2u), n96 = ms_eq64(p4, 0x96u), n81 = ms_eq64(p4, 0x81u);
    const uint32_t nx0 = x[b0 + 64], nx1 = x[b0 + 65];               // the two bytes behind the word
    const unsigned long long n96x = (n96 >> 1) | ((unsigned long long)(nx0 == 0x96u) << 63);
    const unsigned long long n81x = (n81 >> 2) | ((unsigned long long)(nx0 == 0x81u) << 62) | ((unsigned long long)(nx1 == 0x81u) << 63);
    const unsigned long long bars = e2 & n96x & n81x;
    unsigned long long m = bars;
    if (!split) {
        // "▁" in front: a bar three bytes earlier, in this word or at the last three bytes of the word in front
        unsigned long long prev = bars << 3;
        if (w > 0) {
            if (ms_is_bar(x + b0 - 3)) prev |= 1ull;
            if (ms_is_bar(x + b0 - 2)) prev |= 2ull;
            if (ms_is_bar(x + b0 - 1)) prev |= 4ull;
        }
        m &= ~prev;
    }
    m |= pmask[w];
    if (n - b0 < 64) m &= (1ull << (n - b0)) - 1ull;
    startmask[w] = m;
}

// With word ids over whole pieces (no split): the word id of a pre-token is its PIECE's index in the document.  pt_word[p] = the piece
// starts at or in front of pre-token p's start (pprefix: piece starts in front of every 64-byte word), a lane per mask word.
__global__ __launch_bounds__(256) void k_ms_piece_rank(const unsigned long long* __restrict__ startmask, const uint32_t* __restrict__ wprefix,
                                                       const unsigned long long* __restrict__ pmask, const uint32_t* __restrict__ pprefix,
                                                       int64_t n_host, const int64_t* __restrict__ len_dev, uint32_t* __restrict__ pt_word) {
    const int64_t n = len_dev ? *len_dev : n_host;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w > (n >> 6)) return;
    const unsigned long long pm = pmask[w];
    uint32_t r = wprefix[w];
    for (unsigned long long m = startmask[w]; m; m &= m - 1ull, ++r) {
        const int bit = __ffsll(m) - 1;
        pt_word[r] = pprefix[w] + (uint32_t)__popcll(pm & ((2ull << bit) - 1ull));
    }
}
