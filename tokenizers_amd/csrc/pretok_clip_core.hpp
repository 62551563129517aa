// Sequence[Split(the CLIP pattern, Removed, inverted), ByteLevel(add_prefix_space=false)] (CLIPTokenizerFast, the text encoders of Stable
// Diffusion / SDXL, the OpenCLIP conversions; PT_CLIP) as mask algebra over one 64-byte mask word: the word form of pretok_gpt2_core.hpp
// with another rule and a second result.
//
//   's|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+        matched leftmost, first alternative first (Oniguruma)
//
// With `Removed` and `invert` the MATCHES are the pre-tokens and what lies between them -- the \s runs -- belongs to none, so the rule
// writes a start mask and an END mask (a bit on the byte just behind a pre-token's last one, possibly the position n_bytes: the
// convention of pretok_local_core.hpp, which the lookup, the queues and the offsets read).  ByteLevel's own regex behind it matches every
// piece this pattern can cut as one whole: it adds nothing.  With O = a char that is not \s, \p{L} or \p{N}:
//
//   every \p{N} char is a pre-token; a \p{L} run and an O run are one each;
//   a ' opens a contraction only where a match can start at it -- the char in front is not O (or there is none: a document start, either
//   edge of an added-token match) -- and the chars behind it are exactly s, t, m, d, re, ve or ll (lower case, in the same piece); what
//   follows the contraction starts fresh:   'red -> 're d     ''s -> '' s     !'s -> !' s
//
// One char of look-behind and three bytes of look-ahead: purely local, no undecided bytes.  The classes, the halos and what travels
// between lanes are pretok_gpt2_core.hpp's (gpt2_word_classify, gpt2_pack_up / _down, gpt2_take_left / _right); tests/harness/
// clip_harness.cpp runs these functions lane by lane the way k_pretok_clip does and tests/test_clip.py holds the result against the
// reference wheel.  Plain host+device code.
#pragma once
#include <cstdint>

#include "pretok_gpt2_core.hpp"

namespace tkamd {

// The 64 start bits and the 64 end bits of word w: m = its final masks (gpt2_word_classify, then gpt2_take_left), hl / hr = its halos
// (hl as gpt2_take_left made it: its V is not read -- a word in front of byte n_bytes is a whole one).  A word whose first byte is the
// position n_bytes has no byte (m all zero) and may still hold the end bit of the text's last pre-token.  *lead (optional) = "this byte
// exists and is not a continuation byte".
TK_HD void clip_word_masks(const Gpt2Window& m, const Gpt2Halo& hl, const Gpt2Halo& hr, const uint8_t* text, int64_t w, int64_t n_bytes,
                           uint64_t* start, uint64_t* end, uint64_t* lead = nullptr) {
    const int64_t base = w << 6;
    const uint64_t V = m.V, D = m.D, L = m.L, N = m.N, S = m.S, C = m.C;
    const uint64_t LEAD = ~C & V, nD = ~D;
    const uint64_t O = V & ~(L | N | S);
    const uint32_t hV = (w > 0 && base <= n_bytes) ? 0xFFu : 0u;
    const uint32_t hO = hV & ~(hl.L | hl.N | hl.S);
    // (x << 1) with the bit the left halo pushes in: the class of the byte in front, inside the same piece
    const uint64_t pL = ((L << 1) | (hl.L >> 7)) & nD, pO = ((O << 1) | (hO >> 7)) & nD;
    // contractions that are matches: in the word, and in the last three bytes in front of it (they eat into the word).  A match can start at
    // a ' iff the char in front is not an O char of the same piece
    uint64_t CON2 = 0, CON3 = 0;
    uint32_t tCON2 = 0, tCON3 = 0;
    {
        const uint64_t ok = V & nD;
        const uint32_t okR = hr.V & ~hr.D;
        const uint64_t ok1 = (ok >> 1) | ((uint64_t)okR << 63), ok2 = (ok >> 2) | ((uint64_t)okR << 62), L1 = (L >> 1) | ((uint64_t)hr.L << 63);
        for (uint64_t mm = m.AP & ~pO & ok1 & L1; mm; mm &= mm - 1) {
            const int k = __builtin_ctzll(mm);
            const uint32_t b1 = text[base + k + 1], b2 = text[base + k + 2];
            if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') CON2 |= 1ull << k;
            else if ((((b1 == 'r' || b1 == 'v') && b2 == 'e') || (b1 == 'l' && b2 == 'l')) && ((ok2 >> k) & 1ull)) CON3 |= 1ull << k;
        }
        // the same over 16 bits: bits 0..7 the left halo, bits 8..15 the word's first 8 bytes; only bits 5..7 can reach the word
        const uint32_t tL = hl.L | (((uint32_t)L & 0xFFu) << 8), tO = hO | (((uint32_t)O & 0xFFu) << 8), tD = hl.D | (((uint32_t)D & 0xFFu) << 8),
                       tV = hV | (((uint32_t)V & 0xFFu) << 8);
        const uint32_t tok = tV & ~tD, tpO = (tO << 1) & ~tD;
        for (uint32_t mm = hl.AP & hV & ~tpO & (tok >> 1) & (tL >> 1) & 0xE0u; mm; mm &= mm - 1) {
            const int k = __builtin_ctz(mm);
            const uint32_t b1 = text[base + k - 7], b2 = text[base + k - 6];
            if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') tCON2 |= 1u << k;
            else if ((((b1 == 'r' || b1 == 'v') && b2 == 'e') || (b1 == 'l' && b2 == 'l')) && ((tok >> (k + 2)) & 1u)) tCON3 |= 1u << k;
        }
    }
    const uint64_t con = CON2 | CON3;
    const uint32_t tcon = tCON2 | tCON3;
    const uint64_t eaten = (con << 1) | (CON3 << 2) | (uint64_t)((tcon >> 7) | ((tCON3 >> 6) & 3u));
    const uint64_t after = (CON2 << 2) | (CON3 << 3) | (uint64_t)((tCON2 >> 6) | (tCON3 >> 5));
    const uint64_t run = (L & ~pL) | N | (O & ~pO);
    const uint64_t st = LEAD & ~S & (D | (~eaten & (con | after | run)));
    // a pre-token ends in front of byte g -- a lead byte, or the position n_bytes -- if the char in front is kept (not \s) and g starts a
    // pre-token, is a \s char, starts a piece or ends the text
    const int64_t rem = n_bytes - base;
    const uint64_t END = (rem >= 0 && rem < 64) ? 1ull << rem : 0ull;
    const uint64_t kept = L | N | O;
    const uint64_t pK = (kept << 1) | (uint64_t)(((hl.L | hl.N | hO) >> 7) & 1u);
    *start = st;
    *end = (LEAD | END) & pK & (st | S | D | END);
    if (lead) *lead = LEAD;
}

}  // namespace tkamd
