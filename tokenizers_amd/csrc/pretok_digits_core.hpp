// Sequence[Digits(individual_digits), ByteLevel(use_regex=true)] (StarCoder, Granite code, Command-R ...; PT_DIGITS_GPT2) as mask algebra
// over one 64-byte mask word: the word form of pretok_gpt2_core.hpp with one more mask.
//
//   Digits (pre_tokenizers/digits.rs) splits on char::is_numeric -- Isolated when individual_digits (every numeric char a piece), else
//   Contiguous (every maximal run of them a piece) -- and a Sequence hands each piece to the GPT-2 regex as if it were the whole text.
//
// With E = "a piece starts at this byte", E behaves like the document-start mask D wherever gpt2_word_starts reads D: nothing in front of
// here (contractions, the " ?" attachment), and the text ends in front of here (the \s+(?!\S) lookahead, a contraction's letters).  So
// the rule is gpt2_word_starts with D | E in place of D, in the word and in both halos, and everything here is about E:
//
//   Nr = the byte belongs to a char::is_numeric char (UC_RUST_N of the first class table, spread over the char's bytes as L / N / S are;
//        the ASCII digits for ASCII).  It is NOT the N of the GPT-2 classes: thirteen chars are numeric for Rust and not \p{N} for the
//        regex engine, and inside a piece the regex keeps its own classes.
//   pNr = Nr << 1: the byte in front is the last byte of a numeric char.
//   E = lead & (Nr | pNr)   individual digits: a numeric char starts a piece and ends one
//   E = lead & (Nr ^ pNr)   contiguous: only where a run begins or ends
//
// E of a byte needs Nr of that byte and of the one in front, so Nr travels where L / N / S travel: in the spill (a numeric char of 2..4
// bytes across a word edge), in the `up` word (the spill's three bits and the last byte's bit in bits 57..60, free in gpt2_pack_up's
// layout; the D field carries D | E of the word's last 8 bytes, which the word knows by itself) and in a second 32-bit `down` word (the
// first 8 bytes' Nr as classified: their E also needs the spill and the last byte of the word that receives it).
// tests/harness/digits_harness.cpp runs these functions lane by lane the way k_pretok_digits does; tests/test_digits.py holds the result
// against the reference wheel.  Plain host+device code.
#pragma once
#include <cstdint>

#include "pretok_gpt2_core.hpp"

namespace tkamd {

struct DigitsSpill {
    Gpt2Spill g;
    uint32_t Nr;        // bits 0..2: as g.L / g.N / g.S; bit 3: the word's last byte is numeric
};

// piece starts among the bytes of Nr, p_in = the byte in front of bit 0 is numeric (lead: first bytes of chars; T: uint64_t or uint32_t)
template <bool INDIVIDUAL, class T>
TK_HD T digits_edges(T Nr, T p_in, T lead) {
    const T pNr = (T)(Nr << 1) | p_in;
    return lead & (INDIVIDUAL ? (Nr | pNr) : (Nr ^ pNr));
}

// gpt2_word_classify with the Nr mask (*Nr_out, & V) and its spill next to the regex's classes
TK_HD DigitsSpill digits_word_classify(const uint8_t* text, int64_t n_bytes, const uint64_t* docmask, const Gpt2Flags* lut, int64_t w,
                                       const uint16_t* uc1, const uint8_t* uc2, Gpt2Window& m, uint64_t* Nr_out) {
    DigitsSpill sp{{0, 0, 0}, 0};
    const int64_t base = w << 6;
    if (base >= n_bytes) {
        m.L = m.N = m.S = m.SP = m.C = m.AP = m.MU = m.V = m.D = 0;
        *Nr_out = 0;
        return sp;
    }
    uint32_t wd[16];
    {
        const uint8_t* p = text + base;
        const LaneChunk16 c0 = *(const LaneChunk16*)p, c1 = *(const LaneChunk16*)(p + 16), c2 = *(const LaneChunk16*)(p + 32), c3 = *(const LaneChunk16*)(p + 48);
        wd[0] = c0.a; wd[1] = c0.b; wd[2] = c0.c; wd[3] = c0.d; wd[4] = c1.a; wd[5] = c1.b; wd[6] = c1.c; wd[7] = c1.d;
        wd[8] = c2.a; wd[9] = c2.b; wd[10] = c2.c; wd[11] = c2.d; wd[12] = c3.a; wd[13] = c3.b; wd[14] = c3.c; wd[15] = c3.d;
    }
    gpt2_word_flags(wd, lut, m);
    const int64_t rem = n_bytes - base;
    const uint64_t V = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
    uint64_t L = m.L, N = m.N, S = m.S, Nr = m.N;            // (the table's N flag of a byte is the ASCII digits: numeric for both)
    for (uint64_t mm = m.MU & V; mm; mm &= mm - 1) {
        const int k = __builtin_ctzll(mm);
        const uint8_t* p = text + base + k;
        const uint32_t b0 = p[0];
        uint32_t cp, len;
        if (b0 < 0xE0u) { len = 2; cp = ((b0 & 0x1Fu) << 6) | (p[1] & 0x3Fu); }
        else if (b0 < 0xF0u) { len = 3; cp = ((b0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); }
        else { len = 4; cp = ((b0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); }
        const uint32_t f = cp >= 0x110000u ? 0u : uc2[((uint32_t)uc1[cp >> 8] << 8) | (cp & 255u)];
        const uint64_t ones = (1ull << len) - 1ull, span = ones << k;
        const uint32_t over = k + (int)len > 64 ? (uint32_t)(ones >> (64 - k)) : 0u;
        if (f & UC_RUST_N) { Nr |= span; sp.Nr |= over; }
        if (f & UC_ONIG_L) { L |= span; sp.g.L |= over; }
        else if (f & UC_ONIG_N) { N |= span; sp.g.N |= over; }
        else if (f & UC_ONIG_S) { S |= span; sp.g.S |= over; }
    }
    m.L = L & V; m.N = N & V; m.S = S & V; m.SP &= V; m.C &= V; m.AP &= V; m.MU &= V;
    m.V = V;
    m.D = docmask[w] & V;
    Nr &= V;
    sp.Nr |= (uint32_t)(Nr >> 63) << 3;
    *Nr_out = Nr;
    return sp;
}

// gpt2_halo_classify with Nr: the 8 bytes [pos, pos + 8), pos a multiple of 8 with 8 <= pos < n_bytes.  h.D comes back as D | E of the
// 8 bytes (what a word's `up` carries); *Nr8 = their Nr (what a word's second `down` carries).  Code points that begin up to FOUR bytes
// in front of pos are looked at, one more than the regex's classes need: the byte in front of pos decides E of pos.
template <bool INDIVIDUAL>
TK_HD Gpt2Halo digits_halo_classify(const uint8_t* text, int64_t n_bytes, const uint64_t* docmask, const Gpt2Flags* lut, int64_t pos,
                                    const uint16_t* uc1, const uint8_t* uc2, DigitsSpill* spill, uint32_t* Nr8) {
    // bit b of every mask here = byte pos - 8 + b: bits 4..7 are the four bytes in front, 8..15 the halo, 16..18 the spill
    const LaneChunk16 c = *(const LaneChunk16*)(text + pos - 8);
    const uint32_t wd[4] = {c.a, c.b, c.c, c.d};
    uint32_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 4; k < 16; ++k) {
        const Gpt2Flags e = lut[(wd[k >> 2] >> (8 * (k & 3))) & 0xFFu];
        if (k < 8) { a0 |= e.x << k; b0 |= e.y << k; }
        else { a1 |= e.x << (k - 8); b1 |= e.y << (k - 8); }
    }
    const int64_t rem = n_bytes - (pos - 8);
    const uint32_t V = rem >= 16 ? 0xFFFFu : ((1u << rem) - 1u);
    uint32_t L = (a0 & 0xFFu) | ((a1 & 0xFFu) << 8), N = ((a0 >> 8) & 0xFFu) | (((a1 >> 8) & 0xFFu) << 8),
             S = ((a0 >> 16) & 0xFFu) | (((a1 >> 16) & 0xFFu) << 8);
    uint32_t Nr = N;
    const uint32_t MU = ((b0 >> 16) & 0xFFu) | (((b1 >> 16) & 0xFFu) << 8);
    for (uint32_t mm = MU & V; mm; mm &= mm - 1) {
        const int k = __builtin_ctz(mm);
        const uint8_t* p = text + pos - 8 + k;
        const uint32_t c0 = p[0];
        uint32_t cp, len;
        if (c0 < 0xE0u) { len = 2; cp = ((c0 & 0x1Fu) << 6) | (p[1] & 0x3Fu); }
        else if (c0 < 0xF0u) { len = 3; cp = ((c0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); }
        else { len = 4; cp = ((c0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); }
        const uint32_t f = cp >= 0x110000u ? 0u : uc2[((uint32_t)uc1[cp >> 8] << 8) | (cp & 255u)];
        const uint32_t span = ((1u << len) - 1u) << k;
        if (f & UC_RUST_N) Nr |= span;
        if (f & UC_ONIG_L) L |= span; else if (f & UC_ONIG_N) N |= span; else if (f & UC_ONIG_S) S |= span;
    }
    const uint32_t V8 = V >> 8;
    const uint32_t C8 = b1 & 0xFFu & V8;
    Gpt2Halo h;
    h.V = V8;
    h.L = (L >> 8) & V8; h.N = (N >> 8) & V8; h.S = (S >> 8) & V8;
    h.SP = (a1 >> 24) & V8; h.C = C8; h.AP = (b1 >> 8) & 0xFFu & V8;
    const uint32_t nr8 = (Nr >> 8) & V8;
    h.D = ((uint32_t)(docmask[pos >> 6] >> (pos & 63)) & V8) | digits_edges<INDIVIDUAL, uint32_t>(nr8, (Nr >> 7) & 1u, V8 & ~C8);
    *Nr8 = nr8;
    spill->g.L = (L >> 16) & 7u; spill->g.N = (N >> 16) & 7u; spill->g.S = (S >> 16) & 7u;
    spill->Nr = ((Nr >> 16) & 7u) | (((nr8 >> 7) & 1u) << 3);
    return h;
}

// gpt2_pack_up's layout (gpt2_take_left reads it) with the four Nr bits in bits 57..60.  Written out, not a call of gpt2_pack_up: with a
// second caller in the translation unit the compiler orders the ORs of k_pretok_gpt2_seq's own pack differently (three instructions of
// its code object; tools/isa_diff.py), and that kernel is to come out as it was.
TK_HD uint64_t digits_pack_up(uint32_t L, uint32_t N, uint32_t S, uint32_t SP, uint32_t AP, uint32_t D, DigitsSpill sp) {
    const uint32_t lo = L | (N << 8) | (S << 16) | (SP << 24);
    const uint32_t hi = AP | (D << 8) | (sp.g.L << 16) | (sp.g.N << 19) | (sp.g.S << 22) | (sp.Nr << 25);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// `up` of a word: that layout with D | E of the word's last 8 bytes in the D field (all of it the word's own: bit 56's E reads bit 55)
// and the four Nr bits of the spill in bits 57..60
template <bool INDIVIDUAL>
TK_HD uint64_t digits_pack_up(const Gpt2Window& m, uint64_t Nr, DigitsSpill sp) {
    const uint32_t E8 = digits_edges<INDIVIDUAL, uint32_t>((uint32_t)(Nr >> 56), (uint32_t)(Nr >> 55) & 1u, (uint32_t)((~m.C & m.V) >> 56));
    return digits_pack_up((uint32_t)(m.L >> 56), (uint32_t)(m.N >> 56), (uint32_t)(m.S >> 56), (uint32_t)(m.SP >> 56), (uint32_t)(m.AP >> 56),
                          (uint32_t)(m.D >> 56) | E8, sp);
}
// (the halo form: h.D holds D | E already)
TK_HD uint64_t digits_pack_up(const Gpt2Halo& h, DigitsSpill sp) { return digits_pack_up(h.L, h.N, h.S, h.SP, h.AP, h.D, sp); }

// the left halo of word w out of the `up` word of word w - 1, the spills into m and Nr, and E of the word into m.D
template <bool INDIVIDUAL>
TK_HD Gpt2Halo digits_take_left(uint64_t up, int64_t w, Gpt2Window& m, uint64_t& Nr) {
    const Gpt2Halo h = gpt2_take_left(up, w, m);
    const uint32_t nr = (uint32_t)(up >> 57) & 15u;
    Nr |= (uint64_t)(nr & 7u) & m.V;
    m.D |= digits_edges<INDIVIDUAL, uint64_t>(Nr, (uint64_t)(nr >> 3), ~m.C & m.V);
    return h;
}
// the right halo of word w out of the two `down` words of word w + 1, the word's own spill and its own last Nr bit
template <bool INDIVIDUAL>
TK_HD Gpt2Halo digits_take_right(uint32_t down, uint32_t down_nr, int64_t w, int64_t n_bytes, DigitsSpill own) {
    Gpt2Halo h = gpt2_take_right(down, w, n_bytes, own.g);
    const uint32_t nr = ((down_nr & 0xFFu) | (own.Nr & 7u)) & h.V;
    h.D = (h.D | digits_edges<INDIVIDUAL, uint32_t>(nr, own.Nr >> 3, h.V & ~h.C)) & h.V;
    return h;
}

}  // namespace tkamd
