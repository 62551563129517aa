// Sequence[Split(Regex " ?[^(\s|[.,!?…。，、।۔،])]+", Isolated), ByteLevel(add_prefix_space=false, use_regex=false)] (BLOOM / BLOOMZ;
// PT_BLOOM) as mask algebra over one 64-byte mask word, in the word form of pretok_gpt2_core.hpp.
//
//   The pattern is " ?" and then one or more chars of a negated class.  Oniguruma reads the nested brackets as a union, so the class
//   leaves out exactly 39 chars: its \s (UC_ONIG_S: 25 chars) and `! ( ) , . ? |`, U+060C, U+06D4, U+0964, U+2026, U+3001, U+3002, U+FF0C
//   (kBloomPunct; `[` and `]` are NOT left out).  Split(Isolated) makes every match a piece and every stretch between two matches a piece
//   (pre_tokenizers/split.rs:76-105), and ByteLevel(use_regex=false) only maps bytes: the pieces are the pre-tokens.
//
// With X = "the char is one of the 39", NX = "it is not" and SP = U+0020, every mask spread over all bytes of a char as L / N / S are
// in the GPT-2 core, a pre-token starts at a char iff
//   D                                the char is the first of its document (or of a segment between added tokens)
//   NX & (X << 1) & ~(SP << 1)       a match begins: a class char behind an X char that is not the space the match takes along
//   SP & (NX >> 1) & ~(D >> 1)       a match begins at its " ?": a space with a class char of the same document behind it
//   X & (NX << 1)                    a match ended in front of here
// The rule looks one BYTE back and one byte ahead, so nothing is undecided and a lane needs of its neighbours only: X and SP of the byte
// in front and the bytes a char of two or three bytes puts on the word behind it (`up`, 5 bits), and X and D of the byte behind (`down`,
// 2 bits).  X of that byte is taken as the word behind classified it alone: SP is one byte wide, so where the rule reads it no char
// straddles the edge.  The byte classes come from a table of this core's own (four flags a byte value, one 32-bit word), the multi-byte
// X chars from UC_BLOOM_X of the first class table, which the loader sets for handles of this kind only.
// tests/harness/bloom_harness.cpp runs these functions lane by lane the way k_pretok_bloom does; tests/test_bloom.py holds the result
// against the reference wheel.  Plain host+device code.  Bit i of every mask = word byte i.
#pragma once
#include <cstdint>

#include "pretok_gpt2_core.hpp"

namespace tkamd {

// the fourteen chars that the class leaves out next to \s
constexpr uint32_t kBloomPunct[14] = {'!', '(', ')', ',', '.', '?', '|', 0x060Cu, 0x06D4u, 0x0964u, 0x2026u, 0x3001u, 0x3002u, 0xFF0Cu};

// flags of one byte value for the caller's 256-entry table: bit 0 X (the ASCII ones), bit 8 U+0020, bit 16 continuation byte, bit 24
// multi-byte lead
TK_HD uint32_t bloom_byte_flags(uint32_t v) {
    const bool sp = v == 0x20u;
    const bool x = sp || (v - 9u < 5u) || v == '!' || v == '(' || v == ')' || v == ',' || v == '.' || v == '?' || v == '|';
    return (x ? 1u : 0u) | (sp ? 1u << 8 : 0u) | ((v & 0xC0u) == 0x80u ? 1u << 16 : 0u) | (v >= 0xC0u ? 1u << 24 : 0u);
}

struct BloomWord {
    uint64_t X, SP, C;      // one of the 39 (all bytes of the char), U+0020, continuation byte
    uint64_t V, D;          // byte exists, byte starts a document
    uint32_t spill;         // bits 0..2: the bytes an X char that begins in this word puts on the next one
};

// UC_BLOOM_X of the code point whose lead byte is p[0] (>= 0xC0), *len = its bytes
TK_HD bool bloom_wide_x(const uint8_t* p, const uint16_t* uc1, const uint8_t* uc2, uint32_t* len) {
    const uint32_t b0 = p[0];
    uint32_t cp;
    if (b0 < 0xE0u) { *len = 2; cp = ((b0 & 0x1Fu) << 6) | (p[1] & 0x3Fu); }
    else if (b0 < 0xF0u) { *len = 3; cp = ((b0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); }
    else { *len = 4; cp = ((b0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); }
    const uint32_t f = cp >= 0x110000u ? 0u : uc2[((uint32_t)uc1[cp >> 8] << 8) | (cp & 255u)];
    return (f & UC_BLOOM_X) != 0;
}

// the masks of word w with its multi-byte chars resolved, V from n_bytes, D = docmask[w]; every mask & V.  What the word in front spills
// into this one is NOT in yet (bloom_word_starts).  A word past the text is all zero.  The deposit is gpt2_word_flags's with one
// accumulator: a group of eight bytes folded from its last byte down, then a 4 x 4 byte transpose a half.
TK_HD void bloom_word_classify(const uint8_t* text, int64_t n_bytes, const uint64_t* docmask, const uint32_t* lut, int64_t w,
                               const uint16_t* uc1, const uint8_t* uc2, BloomWord& m) {
    const int64_t base = w << 6;
    if (base >= n_bytes) {
        m.X = m.SP = m.C = m.V = m.D = 0;
        m.spill = 0;
        return;
    }
    uint32_t wd[16];
    {
        const uint8_t* p = text + base;                      // four 16-byte loads (the last one may end in the text's pad)
        const LaneChunk16 c0 = *(const LaneChunk16*)p, c1 = *(const LaneChunk16*)(p + 16), c2 = *(const LaneChunk16*)(p + 32), c3 = *(const LaneChunk16*)(p + 48);
        wd[0] = c0.a; wd[1] = c0.b; wd[2] = c0.c; wd[3] = c0.d; wd[4] = c1.a; wd[5] = c1.b; wd[6] = c1.c; wd[7] = c1.d;
        wd[8] = c2.a; wd[9] = c2.b; wd[10] = c2.c; wd[11] = c2.d; wd[12] = c3.a; wd[13] = c3.b; wd[14] = c3.c; wd[15] = c3.d;
    }
    uint32_t A[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < 8; ++g) {
        uint32_t acc = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 7; j >= 0; --j) {
            const int k = 8 * g + j;
            acc = (acc << 1) | lut[(wd[k >> 2] >> (8 * (k & 3))) & 0xFFu];
        }
        A[g] = acc;
    }
    uint32_t lo[4], hi[4];
    gpt2_transpose4(A[0], A[1], A[2], A[3], lo[0], lo[1], lo[2], lo[3]);
    gpt2_transpose4(A[4], A[5], A[6], A[7], hi[0], hi[1], hi[2], hi[3]);
    const int64_t rem = n_bytes - base;
    const uint64_t V = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
    uint64_t X = lo[0] | ((uint64_t)hi[0] << 32);
    const uint64_t MU = lo[3] | ((uint64_t)hi[3] << 32);
    uint32_t spill = 0;
    for (uint64_t mm = MU & V; mm; mm &= mm - 1) {
        const int k = __builtin_ctzll(mm);
        uint32_t len;
        if (bloom_wide_x(text + base + k, uc1, uc2, &len)) {
            const uint64_t ones = (1ull << len) - 1ull;
            X |= ones << k;
            if (k + (int)len > 64) spill |= (uint32_t)(ones >> (64 - k));        // the bytes of this char in the next word
        }
    }
    m.X = X & V;
    m.SP = (lo[1] | ((uint64_t)hi[1] << 32)) & V;
    m.C = (lo[2] | ((uint64_t)hi[2] << 32)) & V;
    m.V = V;
    m.D = docmask[w] & V;
    m.spill = spill & 7u;
}

// What a lane hands to the lane of the next word (`up`: bit 0 X and bit 1 SP of the word's last byte, bits 2..4 the spill) and to the
// lane of the word in front (`down`: bit 0 X and bit 1 D of the word's first byte).  V is not passed: it follows from n_bytes.
TK_HD uint32_t bloom_pack_up(const BloomWord& m) { return (uint32_t)(m.X >> 63) | ((uint32_t)(m.SP >> 63) << 1) | (m.spill << 2); }
TK_HD uint32_t bloom_pack_down(const BloomWord& m) { return ((uint32_t)m.X & 1u) | (((uint32_t)m.D & 1u) << 1); }

// The same two words for what lies beyond a workgroup, from the text itself.  `up` of the word that ends in front of byte base (base a
// multiple of 64, 0 < base < n_bytes): its last byte, and the leads among its last four bytes as its own lane resolves them.
TK_HD uint32_t bloom_edge_up(const uint8_t* text, int64_t base, const uint32_t* lut, const uint16_t* uc1, const uint8_t* uc2) {
    const uint32_t last = lut[text[base - 1]];
    uint32_t x = last & 1u, spill = 0;
    for (int d = 1; d <= 4; ++d) {
        const uint8_t* p = text + base - d;
        uint32_t len;
        if (p[0] >= 0xC0u && bloom_wide_x(p, uc1, uc2, &len) && (int)len >= d) {
            x = 1u;
            spill |= ((1u << len) - 1u) >> d;
        }
    }
    return x | (((last >> 8) & 1u) << 1) | ((spill & 7u) << 2);
}
// `down` of the word that begins at byte pos (pos a multiple of 64, pos < n_bytes)
TK_HD uint32_t bloom_edge_down(const uint8_t* text, int64_t pos, const uint64_t* docmask, const uint32_t* lut, const uint16_t* uc1, const uint8_t* uc2) {
    const uint8_t* p = text + pos;
    uint32_t x = lut[p[0]] & 1u, len;
    if (p[0] >= 0xC0u && bloom_wide_x(p, uc1, uc2, &len)) x = 1u;
    return x | (((uint32_t)docmask[pos >> 6] & 1u) << 1);
}

// The 64 start bits of word w: m = its masks (bloom_word_classify), up = the `up` word of word w - 1, down = the `down` word of word
// w + 1 (0 where there is none).  *lead (optional) = "this byte exists and is not a continuation byte", the lead-byte mask char offsets
// count in.
TK_HD uint64_t bloom_word_starts(const BloomWord& m, uint32_t up, uint32_t down, int64_t w, int64_t n_bytes, uint64_t* lead = nullptr) {
    const uint64_t V = m.V, D = m.D, SP = m.SP;
    const uint64_t X = (m.X | (uint64_t)((up >> 2) & 7u)) & V;
    const uint64_t NX = V & ~X, LEAD = V & ~m.C;
    // a word that has a byte has a whole word in front of it; the word behind has a byte iff the text goes on
    const uint64_t lV = (w > 0 && V) ? 1ull : 0ull, rV = n_bytes > ((w + 1) << 6) ? 1ull : 0ull;
    const uint64_t lX = up & 1u, lSP = (up >> 1) & 1u, rX = down & 1u, rD = (down >> 1) & 1u;
    // (x << 1) with the bit the word in front pushes in, (x >> 1) with the bit of the word behind
    const uint64_t pX = (X << 1) | (lX & lV), pSP = (SP << 1) | (lSP & lV), pNX = (NX << 1) | (lV & ~lX);
    const uint64_t nNX = (NX >> 1) | ((rV & ~rX) << 63), nD = (D >> 1) | ((rD & rV) << 63);
    if (lead) *lead = LEAD;
    return LEAD & (D | (NX & pX & ~pSP) | (SP & nNX & ~nD) | (X & pNX));
}

}  // namespace tkamd
