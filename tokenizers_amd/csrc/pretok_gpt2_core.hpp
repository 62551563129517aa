// GPT-2 ByteLevel split as 64-bit mask algebra over one 64-byte window.
//
//   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+        pre_tokenizers/byte_level.rs:43-46
//
// Two forms of the same algebra.  The WINDOW form (first half of this file): a lane owns the 48 bytes [8, 56) of a 64-byte
// window and decides for each of them whether a regex match starts there (the rule only looks <= 4 code
// points back and 3 ahead, so an 8-byte halo is enough and nothing is ever left undecided).  The fused lookup uses it for 48
// bytes anywhere in the text (gpt2_starts_at), and the CPU test tests/test_pretok_core.py runs it (tests/harness/l3_harness.cpp)
// against the sequential matcher of the test tree.  The WORD form (second half) is what k_pretok_gpt2_seq runs: a lane owns one
// 64-byte mask word and takes the halo from its neighbours' masks; tests/test_pretok_gpt2_words.py holds it word for word
// against the window form.  Plain host+device code.  Bit i of every mask = window (word) byte i.
#pragma once
#include <cstdint>

#include "tables.hpp"

namespace tkamd {

constexpr int G2W_HALO = 8;
constexpr int G2W_MAIN = 48;
constexpr uint64_t G2W_MAIN_MASK = 0x00FFFFFFFFFFFF00ull;

struct Gpt2Window {
    uint64_t L, N, S, SP;         // letter, number, whitespace (Oniguruma \s), U+0020      ASCII bytes only on entry
    uint64_t C, AP, MU;           // continuation byte, apostrophe, multi-byte lead
    uint64_t V, D;                // byte exists, byte starts a document
};

// flag words of one byte value for the caller's 256-entry table: bits 0 / 8 / 16 / 24 of .x = L, N, S, SP; bits 0 / 8 / 16
// of .y = continuation, apostrophe, multi-byte lead
struct Gpt2Flags { uint32_t x, y; };
TK_HD Gpt2Flags gpt2_byte_flags(uint32_t v) {
    const uint32_t lower = v | 0x20u;
    const bool isL = v < 0x80u && (lower - 'a' < 26u), isN = (v - '0' < 10u), isS = (v == 0x20u) || (v - 9u < 5u);
    Gpt2Flags f;
    f.x = (isL ? 1u : 0u) | (isN ? 1u << 8 : 0u) | (isS ? 1u << 16 : 0u) | (v == 0x20u ? 1u << 24 : 0u);
    f.y = ((v & 0xC0u) == 0x80u ? 1u : 0u) | (v == '\'' ? 1u << 8 : 0u) | (v >= 0xC0u ? 1u << 16 : 0u);
    return f;
}

// `text + base` is window byte 0 (V says which bytes exist; the text carries TKAMD_TEXT_PAD readable bytes after its end).
// Returns the match starts of window bytes [8, 56) in bits 8..55.
TK_HD uint64_t gpt2_window_starts(Gpt2Window m, const uint8_t* text, int64_t base, const uint16_t* uc1, const uint8_t* uc2) {
    const uint64_t V = m.V, D = m.D & V;
    uint64_t L = m.L, N = m.N, S = m.S;
    const uint64_t C = m.C, SP = m.SP & V;
    // multi-byte code points: class from the Unicode table, spread over the lead and its continuation bytes
    for (uint64_t mm = m.MU & V; mm; mm &= mm - 1) {
        const int k = __builtin_ctzll(mm);
        const uint8_t* p = text + base + k;
        const uint32_t b0 = p[0];
        uint32_t cp, len;
        if (b0 < 0xE0u) { len = 2; cp = ((b0 & 0x1Fu) << 6) | (p[1] & 0x3Fu); }
        else if (b0 < 0xF0u) { len = 3; cp = ((b0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); }
        else { len = 4; cp = ((b0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); }
        const uint32_t f = cp >= 0x110000u ? 0u : uc2[((uint32_t)uc1[cp >> 8] << 8) | (cp & 255u)];
        const uint64_t span = ((1ull << len) - 1ull) << k;
        if (f & UC_ONIG_L) L |= span; else if (f & UC_ONIG_N) N |= span; else if (f & UC_ONIG_S) S |= span;
    }
    L &= V; N &= V; S &= V;
    const uint64_t LEAD = ~C & V, nD = ~D;
    const uint64_t O = V & ~(L | N | S);
    const uint64_t pL = (L << 1) & nD, pN = (N << 1) & nD, pS = (S << 1) & nD, pO = (O << 1) & nD, pSP = (SP << 1) & nD;
    // contraction literals 's 't 'm 'd | 're 've 'll that are match starts
    uint64_t CON2 = 0, CON3 = 0;
    {
        const uint64_t ok = V & nD;                                          // byte exists and continues the document
        const uint64_t cond = D | pL | pN | (pS & ~pSP);
        for (uint64_t mm = m.AP & V & cond & (ok >> 1) & (L >> 1); mm; mm &= mm - 1) {
            const int k = __builtin_ctzll(mm);
            const uint32_t b1 = text[base + k + 1], b2 = text[base + k + 2];
            if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') CON2 |= 1ull << k;
            else if ((((b1 == 'r' || b1 == 'v') && b2 == 'e') || (b1 == 'l' && b2 == 'l')) && k + 2 < 64 && ((ok >> (k + 2)) & 1ull)) CON3 |= 1ull << k;
        }
    }
    const uint64_t con = CON2 | CON3;
    const uint64_t eaten = (con << 1) | (CON3 << 2);
    const uint64_t after = (CON2 << 2) | (CON3 << 3);
    const uint64_t run = (L & ~(pL | pSP)) | (N & ~(pN | pSP)) | (O & ~(pO | pSP));
    const uint64_t wsfirst = S & ~pS;
    // whitespace after whitespace starts a match iff the NEXT code point is a non-space of the same document
    uint64_t Y = (LEAD & ~S & nD) >> 1;
    Y |= (Y & C) >> 1; Y |= (Y & C) >> 1; Y |= (Y & C) >> 1;
    const uint64_t wslast = S & pS & Y;
    return LEAD & (D | (~eaten & (con | after | run | wsfirst | wslast))) & G2W_MAIN_MASK;
}

// ---- the whole lane: loads, flag deposit, masks of valid bytes / document starts, the algebra above ------------------
// A lane owns bytes [48 * lane, 48 * lane + 48) of the text; its window starts 8 bytes earlier.  `text` must be readable up to
// n_bytes + TKAMD_TEXT_PAD; `lut` is the 256-entry table of gpt2_byte_flags (an LDS copy in the kernel); `docmask` has one bit
// per byte, (n_bytes_host >> 6) + 1 words.  Returns the 48 start bits (bit 0 = the lane's first byte), 0 past the text.
struct __attribute__((packed, aligned(8))) LaneChunk16 { uint32_t a, b, c, d; };    // 16-byte load at 8-byte alignment
struct __attribute__((packed, aligned(8))) LaneChunk8 { uint32_t a, b; };

// flag deposit: the window's 64 bytes (16 dwords, little endian) -> the seven byte-class masks of Gpt2Window.  The table entries are
// one-hot flags 8 bits apart, so one shift-or per byte deposits a flag into four masks at once and every eight bytes the finished
// groups move into the 64-bit masks.  (V and D are the caller's.)
TK_HD void gpt2_window_flags(const uint32_t* w, const Gpt2Flags* lut, Gpt2Window& m) {
    m.L = m.N = m.S = m.SP = m.C = m.AP = m.MU = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < 8; ++g) {
        uint32_t accA = 0, accB = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * g + j;
            const Gpt2Flags e = lut[(w[k >> 2] >> (8 * (k & 3))) & 0xFFu];
            accA |= e.x << j;
            accB |= e.y << j;
        }
        m.L |= (uint64_t)(accA & 0xFFu) << (8 * g);
        m.N |= (uint64_t)((accA >> 8) & 0xFFu) << (8 * g);
        m.S |= (uint64_t)((accA >> 16) & 0xFFu) << (8 * g);
        m.SP |= (uint64_t)(accA >> 24) << (8 * g);
        m.C |= (uint64_t)(accB & 0xFFu) << (8 * g);
        m.AP |= (uint64_t)((accB >> 8) & 0xFFu) << (8 * g);
        m.MU |= (uint64_t)((accB >> 16) & 0xFFu) << (8 * g);
    }
}
// which bytes of the window [base, base + 64) exist, and which of them start a document (docmask: one bit per byte of the text,
// n_words_host words)
TK_HD void gpt2_window_valid(int64_t base, int64_t n_bytes, int64_t n_words_host, const uint64_t* docmask, Gpt2Window& m) {
    const int vlo = base < 0 ? (int)-base : 0;
    const int64_t rem = n_bytes - base;
    m.V = (rem >= 64 ? ~0ull : ((1ull << rem) - 1ull)) & (~0ull << vlo);
    if (base < 0) m.D = docmask[0] << (int)-base;
    else {
        const int64_t wi = base >> 6;
        const int sh = (int)(base & 63);
        m.D = docmask[wi] >> sh;
        if (sh && wi + 1 < n_words_host) m.D |= docmask[wi + 1] << (64 - sh);
    }
    m.D &= m.V;
}

// (lead, optional: the lane's 48 bits of "this byte exists and is not a continuation byte" -- the lead-byte mask char offsets count in,
// kernels/output.hip k_leadmask: the window's flags hold it already)
TK_HD uint64_t gpt2_lane_starts(const uint8_t* text, int64_t n_bytes, int64_t n_words_host, const uint64_t* docmask, const Gpt2Flags* lut,
                                int64_t lane, const uint16_t* uc1, const uint8_t* uc2, uint64_t* lead = nullptr) {
    const int64_t a = lane * G2W_MAIN;                       // first byte this lane decides
    const int64_t base = a - G2W_HALO;                       // window = [base, base + 64)
    if (lead) *lead = 0;
    if (a >= n_bytes) return 0;
    uint32_t w[16];
    {
        // four 16-byte loads (8-byte aligned: gfx950 takes dwordx4 at any alignment); only lane 0's window starts before the text
        LaneChunk16 c0{0, 0, 0, 0};
        if (base >= 0) c0 = *(const LaneChunk16*)(text + base);
        else { const LaneChunk8 t = *(const LaneChunk8*)text; c0.c = t.a; c0.d = t.b; }
        const LaneChunk16 c1 = *(const LaneChunk16*)(text + base + 16), c2 = *(const LaneChunk16*)(text + base + 32),
                          c3 = *(const LaneChunk16*)(text + base + 48);
        w[0] = c0.a; w[1] = c0.b; w[2] = c0.c; w[3] = c0.d; w[4] = c1.a; w[5] = c1.b; w[6] = c1.c; w[7] = c1.d;
        w[8] = c2.a; w[9] = c2.b; w[10] = c2.c; w[11] = c2.d; w[12] = c3.a; w[13] = c3.b; w[14] = c3.c; w[15] = c3.d;
    }
    Gpt2Window m;
    gpt2_window_valid(base, n_bytes, n_words_host, docmask, m);      // valid positions of the window and their document-start bits
    gpt2_window_flags(w, lut, m);
    if (lead) *lead = ((m.V & ~m.C) >> G2W_HALO) & ((1ull << G2W_MAIN) - 1ull);
    return (gpt2_window_starts(m, text, base, uc1, uc2) >> G2W_HALO) & ((1ull << G2W_MAIN) - 1ull);
}

// The same for 48 bytes that start ANYWHERE in the text (first byte a >= 0): byte-unaligned loads.  The fused lookup (kernels/lookup.hip)
// uses it off its main path -- a pre-token that runs on beyond the staged tile, a look-back that computes a missing tile's count.
struct __attribute__((packed, aligned(1))) LaneChunk16u { uint32_t a, b, c, d; };
TK_HD uint64_t gpt2_starts_at(const uint8_t* text, int64_t a, int64_t n_bytes, int64_t n_words_host, const uint64_t* docmask, const Gpt2Flags* lut,
                              const uint16_t* uc1, const uint8_t* uc2) {
    if (a >= n_bytes) return 0;
    const int64_t base = a - G2W_HALO;
    uint32_t w[16];
    if (base >= 0) {
        for (int k = 0; k < 4; ++k) {
            const LaneChunk16u c = *(const LaneChunk16u*)(text + base + 16 * k);
            w[4 * k] = c.a; w[4 * k + 1] = c.b; w[4 * k + 2] = c.c; w[4 * k + 3] = c.d;
        }
    } else {                                                 // (the text's first bytes: the window starts in front of it)
        for (int k = 0; k < 16; ++k) w[k] = 0;
        for (int k = (int)-base; k < 64; ++k) w[k >> 2] |= (uint32_t)text[base + k] << (8 * (k & 3));
    }
    Gpt2Window m;
    gpt2_window_valid(base, n_bytes, n_words_host, docmask, m);
    gpt2_window_flags(w, lut, m);
    return (gpt2_window_starts(m, text, base, uc1, uc2) >> G2W_HALO) & ((1ull << G2W_MAIN) - 1ull);
}

// ---- the word-aligned form: one lane = one 64-bit word of the start mask = text bytes [64 w, 64 w + 64) -------------------------------
// k_pretok_gpt2_seq runs this one.  A lane classifies exactly its own 64 bytes (no byte is classified twice), resolves its multi-byte code
// points, and only then looks at its neighbours: 8 bytes of their FINAL masks each way (the halo of the window form, G2W_HALO), which the
// kernel passes between lanes as one 64-bit word up and one 32-bit word down.  The algebra is gpt2_window_starts's, with the bits a shift
// pulls in from outside the word taken from the halos.  tests/harness/g2w_harness.cpp runs these functions lane by lane the way the
// kernel does and compares every mask word with gpt2_lane_starts's.

// what a code point whose lead byte is one of the word's last three bytes puts on the first bytes of the NEXT word (bits 0..2)
struct Gpt2Spill { uint32_t L, N, S; };
// 8 bytes of a neighbouring word, 8 bits a mask.  Left halo: bit 7 = the byte in front of the word; right halo: bit 0 = the byte behind it.
// gpt2_word_starts reads L N S SP AP V D of the left one and L S C V D of the right one; an absent neighbour is all zero.
struct Gpt2Halo { uint32_t L, N, S, SP, C, AP, V, D; };

// The flag deposit of gpt2_window_flags with fewer instructions for the same masks.  A group of eight bytes is folded from its last byte
// down, acc = (acc << 1) | flags: one shift-or per byte and accumulator, and a flag still ends up at bit j of its 8-bit field.  The groups'
// fields are then gathered a 4 x 4 byte transpose at a time (two levels of two-word byte merges) instead of a field at a time.
TK_HD void gpt2_transpose4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t& f0, uint32_t& f1, uint32_t& f2, uint32_t& f3) {
    // word g holds field f of group g in byte f; out: word f holds group g's field in byte g
    const uint32_t t0 = (a0 & 0xFFu) | ((a1 & 0xFFu) << 8) | ((a0 & 0xFF00u) << 8) | ((a1 & 0xFF00u) << 16);        // a0.0 a1.0 a0.1 a1.1
    const uint32_t t1 = ((a0 >> 16) & 0xFFu) | ((a1 >> 8) & 0xFF00u) | ((a0 >> 8) & 0xFF0000u) | (a1 & 0xFF000000u);   // a0.2 a1.2 a0.3 a1.3
    const uint32_t t2 = (a2 & 0xFFu) | ((a3 & 0xFFu) << 8) | ((a2 & 0xFF00u) << 8) | ((a3 & 0xFF00u) << 16);
    const uint32_t t3 = ((a2 >> 16) & 0xFFu) | ((a3 >> 8) & 0xFF00u) | ((a2 >> 8) & 0xFF0000u) | (a3 & 0xFF000000u);
    f0 = (t0 & 0xFFFFu) | (t2 << 16);
    f1 = (t0 >> 16) | (t2 & 0xFFFF0000u);
    f2 = (t1 & 0xFFFFu) | (t3 << 16);
    f3 = (t1 >> 16) | (t3 & 0xFFFF0000u);
}
TK_HD void gpt2_word_flags(const uint32_t* w, const Gpt2Flags* lut, Gpt2Window& m) {
    uint32_t A[8], B[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < 8; ++g) {
        uint32_t accA = 0, accB = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 7; j >= 0; --j) {
            const int k = 8 * g + j;
            const Gpt2Flags e = lut[(w[k >> 2] >> (8 * (k & 3))) & 0xFFu];
            accA = (accA << 1) | e.x;
            accB = (accB << 1) | e.y;
        }
        A[g] = accA;
        B[g] = accB;
    }
    uint32_t lo[4], hi[4];
    gpt2_transpose4(A[0], A[1], A[2], A[3], lo[0], lo[1], lo[2], lo[3]);
    gpt2_transpose4(A[4], A[5], A[6], A[7], hi[0], hi[1], hi[2], hi[3]);
    m.L = lo[0] | ((uint64_t)hi[0] << 32); m.N = lo[1] | ((uint64_t)hi[1] << 32);
    m.S = lo[2] | ((uint64_t)hi[2] << 32); m.SP = lo[3] | ((uint64_t)hi[3] << 32);
    gpt2_transpose4(B[0], B[1], B[2], B[3], lo[0], lo[1], lo[2], lo[3]);
    gpt2_transpose4(B[4], B[5], B[6], B[7], hi[0], hi[1], hi[2], hi[3]);
    m.C = lo[0] | ((uint64_t)hi[0] << 32); m.AP = lo[1] | ((uint64_t)hi[1] << 32); m.MU = lo[2] | ((uint64_t)hi[2] << 32);
}

// the seven class masks of word w with its multi-byte code points resolved, V from n_bytes, D = docmask[w]; every mask & V.  What the word
// in front spills into this one is NOT in yet (gpt2_take_left).  A word past the text is all zero.
TK_HD Gpt2Spill gpt2_word_classify(const uint8_t* text, int64_t n_bytes, const uint64_t* docmask, const Gpt2Flags* lut, int64_t w,
                                   const uint16_t* uc1, const uint8_t* uc2, Gpt2Window& m) {
    Gpt2Spill sp{0, 0, 0};
    const int64_t base = w << 6;
    if (base >= n_bytes) {
        m.L = m.N = m.S = m.SP = m.C = m.AP = m.MU = m.V = m.D = 0;
        return sp;
    }
    uint32_t wd[16];
    {
        const uint8_t* p = text + base;                      // four 16-byte loads, 16-byte aligned when the text is (the last one may end in the text's pad)
        const LaneChunk16 c0 = *(const LaneChunk16*)p, c1 = *(const LaneChunk16*)(p + 16), c2 = *(const LaneChunk16*)(p + 32), c3 = *(const LaneChunk16*)(p + 48);
        wd[0] = c0.a; wd[1] = c0.b; wd[2] = c0.c; wd[3] = c0.d; wd[4] = c1.a; wd[5] = c1.b; wd[6] = c1.c; wd[7] = c1.d;
        wd[8] = c2.a; wd[9] = c2.b; wd[10] = c2.c; wd[11] = c2.d; wd[12] = c3.a; wd[13] = c3.b; wd[14] = c3.c; wd[15] = c3.d;
    }
    gpt2_word_flags(wd, lut, m);
    const int64_t rem = n_bytes - base;
    const uint64_t V = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
    uint64_t L = m.L, N = m.N, S = m.S;
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
        const uint32_t over = k + (int)len > 64 ? (uint32_t)(ones >> (64 - k)) : 0u;           // the bytes of this code point in the next word
        if (f & UC_ONIG_L) { L |= span; sp.L |= over; }
        else if (f & UC_ONIG_N) { N |= span; sp.N |= over; }
        else if (f & UC_ONIG_S) { S |= span; sp.S |= over; }
    }
    m.L = L & V; m.N = N & V; m.S = S & V; m.SP &= V; m.C &= V; m.AP &= V; m.MU &= V;
    m.V = V;
    m.D = docmask[w] & V;
    return sp;
}

// The same for the 8 bytes [pos, pos + 8) alone, pos a multiple of 8 with 8 <= pos < n_bytes: what the first and the last lane of a
// workgroup know of the word beyond it.  Code points that begin up to three bytes in front of pos are resolved too; *spill is what the
// 8 bytes put on the bytes behind them.
TK_HD Gpt2Halo gpt2_halo_classify(const uint8_t* text, int64_t n_bytes, const uint64_t* docmask, const Gpt2Flags* lut, int64_t pos,
                                  const uint16_t* uc1, const uint8_t* uc2, Gpt2Spill* spill) {
    // bit b of every mask here = byte pos - 8 + b: bits 5..7 are the three bytes in front, 8..15 the halo, 16..18 the spill
    const LaneChunk16 c = *(const LaneChunk16*)(text + pos - 8);
    const uint32_t wd[4] = {c.a, c.b, c.c, c.d};
    uint32_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 5; k < 16; ++k) {
        const Gpt2Flags e = lut[(wd[k >> 2] >> (8 * (k & 3))) & 0xFFu];
        if (k < 8) { a0 |= e.x << k; b0 |= e.y << k; }
        else { a1 |= e.x << (k - 8); b1 |= e.y << (k - 8); }
    }
    const int64_t rem = n_bytes - (pos - 8);
    const uint32_t V = rem >= 16 ? 0xFFFFu : ((1u << rem) - 1u);
    uint32_t L = (a0 & 0xFFu) | ((a1 & 0xFFu) << 8), N = ((a0 >> 8) & 0xFFu) | (((a1 >> 8) & 0xFFu) << 8),
             S = ((a0 >> 16) & 0xFFu) | (((a1 >> 16) & 0xFFu) << 8);
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
        if (f & UC_ONIG_L) L |= span; else if (f & UC_ONIG_N) N |= span; else if (f & UC_ONIG_S) S |= span;
    }
    const uint32_t V8 = V >> 8;
    Gpt2Halo h;
    h.V = V8;
    h.L = (L >> 8) & V8; h.N = (N >> 8) & V8; h.S = (S >> 8) & V8;
    h.SP = (a1 >> 24) & V8; h.C = b1 & 0xFFu & V8; h.AP = (b1 >> 8) & 0xFFu & V8;
    h.D = (uint32_t)(docmask[pos >> 6] >> (pos & 63)) & V8;
    spill->L = (L >> 16) & 7u; spill->N = (N >> 16) & 7u; spill->S = (S >> 16) & 7u;
    return h;
}

// What a lane hands to the lane of the next word (`up`: the top 8 bits of L N S SP AP D in bytes 0..5, the spill in bits 48..56) and to
// the lane of the word in front (`down`: the low 8 bits of L S C D).  V is not passed: it follows from n_bytes.
TK_HD uint64_t gpt2_pack_up(uint32_t L, uint32_t N, uint32_t S, uint32_t SP, uint32_t AP, uint32_t D, Gpt2Spill sp) {
    return (uint64_t)(L | (N << 8) | (S << 16) | (SP << 24)) | ((uint64_t)(AP | (D << 8) | (sp.L << 16) | (sp.N << 19) | (sp.S << 22)) << 32);
}
TK_HD uint64_t gpt2_pack_up(const Gpt2Window& m, Gpt2Spill sp) {
    return gpt2_pack_up((uint32_t)(m.L >> 56), (uint32_t)(m.N >> 56), (uint32_t)(m.S >> 56), (uint32_t)(m.SP >> 56), (uint32_t)(m.AP >> 56),
                        (uint32_t)(m.D >> 56), sp);
}
TK_HD uint32_t gpt2_pack_down(uint32_t L, uint32_t S, uint32_t C, uint32_t D) { return L | (S << 8) | (C << 16) | (D << 24); }
TK_HD uint32_t gpt2_pack_down(const Gpt2Window& m) {
    return gpt2_pack_down((uint32_t)m.L & 0xFFu, (uint32_t)m.S & 0xFFu, (uint32_t)m.C & 0xFFu, (uint32_t)m.D & 0xFFu);
}
// the left halo of word w out of the `up` word of word w - 1 (0 where there is none); the spill goes into m
TK_HD Gpt2Halo gpt2_take_left(uint64_t up, int64_t w, Gpt2Window& m) {
    const uint32_t lo = (uint32_t)up, hi = (uint32_t)(up >> 32);
    Gpt2Halo h;
    h.L = lo & 0xFFu; h.N = (lo >> 8) & 0xFFu; h.S = (lo >> 16) & 0xFFu; h.SP = lo >> 24;
    h.AP = hi & 0xFFu; h.D = (hi >> 8) & 0xFFu; h.C = 0;
    h.V = (w > 0 && m.V) ? 0xFFu : 0u;                       // a word that has a byte has a whole word in front of it
    m.L |= (uint64_t)((hi >> 16) & 7u) & m.V; m.N |= (uint64_t)((hi >> 19) & 7u) & m.V; m.S |= (uint64_t)((hi >> 22) & 7u) & m.V;
    return h;
}
// the right halo of word w out of the `down` word of word w + 1 (0 where there is none) and the word's own spill
TK_HD Gpt2Halo gpt2_take_right(uint32_t down, int64_t w, int64_t n_bytes, Gpt2Spill own) {
    const int64_t rem = n_bytes - ((w + 1) << 6);
    Gpt2Halo h;
    h.V = rem >= 8 ? 0xFFu : rem > 0 ? ((1u << rem) - 1u) : 0u;
    h.L = ((down & 0xFFu) | own.L) & h.V; h.S = (((down >> 8) & 0xFFu) | own.S) & h.V; h.N = own.N & h.V;
    h.C = (down >> 16) & 0xFFu; h.D = down >> 24;
    h.SP = 0; h.AP = 0;
    return h;
}

// The 64 start bits of word w: m = its final masks (gpt2_word_classify, then gpt2_take_left), hl / hr = its halos.  *lead (optional) =
// "this byte exists and is not a continuation byte", the lead-byte mask char offsets count in.
TK_HD uint64_t gpt2_word_starts(const Gpt2Window& m, const Gpt2Halo& hl, const Gpt2Halo& hr, const uint8_t* text, int64_t w,
                                uint64_t* lead = nullptr) {
    const int64_t base = w << 6;
    const uint64_t V = m.V, D = m.D, L = m.L, N = m.N, S = m.S, C = m.C, SP = m.SP;
    const uint64_t LEAD = ~C & V, nD = ~D;
    const uint64_t O = V & ~(L | N | S);
    const uint32_t hO = hl.V & ~(hl.L | hl.N | hl.S);
    // (x << 1) with the bit the left halo pushes in
    const uint64_t pL = ((L << 1) | (hl.L >> 7)) & nD, pN = ((N << 1) | (hl.N >> 7)) & nD, pS = ((S << 1) | (hl.S >> 7)) & nD,
                   pO = ((O << 1) | (hO >> 7)) & nD, pSP = ((SP << 1) | (hl.SP >> 7)) & nD;
    // contraction literals that are match starts: in the word, and in the last three bytes in front of it (they eat into the word)
    uint64_t CON2 = 0, CON3 = 0;
    uint32_t tCON2 = 0, tCON3 = 0;
    {
        const uint64_t ok = V & nD;
        const uint32_t okR = hr.V & ~hr.D;
        const uint64_t ok1 = (ok >> 1) | ((uint64_t)okR << 63), ok2 = (ok >> 2) | ((uint64_t)okR << 62), L1 = (L >> 1) | ((uint64_t)hr.L << 63);
        const uint64_t cond = D | pL | pN | (pS & ~pSP);
        for (uint64_t mm = m.AP & cond & ok1 & L1; mm; mm &= mm - 1) {
            const int k = __builtin_ctzll(mm);
            const uint32_t b1 = text[base + k + 1], b2 = text[base + k + 2];
            if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') CON2 |= 1ull << k;
            else if ((((b1 == 'r' || b1 == 'v') && b2 == 'e') || (b1 == 'l' && b2 == 'l')) && ((ok2 >> k) & 1ull)) CON3 |= 1ull << k;
        }
        // the same over 16 bits: bits 0..7 the left halo, bits 8..15 the word's first 8 bytes; only bits 5..7 can reach the word
        const uint32_t tL = hl.L | (((uint32_t)L & 0xFFu) << 8), tN = hl.N | (((uint32_t)N & 0xFFu) << 8), tS = hl.S | (((uint32_t)S & 0xFFu) << 8),
                       tSP = hl.SP | (((uint32_t)SP & 0xFFu) << 8), tD = hl.D | (((uint32_t)D & 0xFFu) << 8), tV = hl.V | (((uint32_t)V & 0xFFu) << 8);
        const uint32_t tnD = ~tD, tok = tV & tnD;
        const uint32_t tpL = (tL << 1) & tnD, tpN = (tN << 1) & tnD, tpS = (tS << 1) & tnD, tpSP = (tSP << 1) & tnD;
        const uint32_t tcond = tD | tpL | tpN | (tpS & ~tpSP);
        for (uint32_t mm = hl.AP & hl.V & tcond & (tok >> 1) & (tL >> 1) & 0xE0u; mm; mm &= mm - 1) {
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
    const uint64_t run = (L & ~(pL | pSP)) | (N & ~(pN | pSP)) | (O & ~(pO | pSP));
    const uint64_t wsfirst = S & ~pS;
    // whitespace after whitespace starts a match iff the NEXT code point is a non-space of the same document: (x >> n) with the bits the
    // right halo pushes in, the three `Y |= (Y & C) >> 1` of the window form written out
    const uint64_t Z = LEAD & ~S & nD;
    const uint32_t ZR = hr.V & ~hr.C & ~hr.S & ~hr.D, CR = hr.C & hr.V;
    const uint64_t C1 = (C >> 1) | ((uint64_t)CR << 63), C2 = (C >> 2) | ((uint64_t)CR << 62), C3 = (C >> 3) | ((uint64_t)CR << 61);
    const uint64_t Z1 = (Z >> 1) | ((uint64_t)ZR << 63), Z2 = (Z >> 2) | ((uint64_t)ZR << 62), Z3 = (Z >> 3) | ((uint64_t)ZR << 61),
                   Z4 = (Z >> 4) | ((uint64_t)ZR << 60);
    const uint64_t Y = Z1 | (C1 & (Z2 | (C2 & (Z3 | (C3 & Z4)))));
    const uint64_t wslast = S & pS & Y;
    if (lead) *lead = LEAD;
    return LEAD & (D | (~eaten & (con | after | run | wsfirst | wslast)));
}

}  // namespace tkamd
