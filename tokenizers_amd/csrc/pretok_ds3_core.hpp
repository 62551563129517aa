// The DeepSeek-V3 / R1 chain of three Splits in front of ByteLevel(use_regex=false), as 64-bit mask algebra over ONE 64-byte window and
// as a sequential per-document matcher.
//
//   1  \p{N}{1,3}
//   2  [U+4E00-U+9FA5 U+3040-U+309F U+30A0-U+30FF]+
//   3  [!"#$%&'()*+,\-./:;<=>?@\[\\\]^_`{|}~][A-Za-z]+ | [^\r\n\p{L}\p{P}\p{S}]?[\p{L}\p{M}]+ |  ?[\p{P}\p{S}]+[\r\n]* | \s*[\r\n]+ | \s+(?!\S) | \s+
//
// pre_tokenizers/sequence.rs hands every piece one Split leaves to the next one, so the chain is NOT the alternation of the three: an edge
// an earlier stage made is the end of the text for a later one.  Stage 1 cuts every digit run into threes from its start, stage 2 isolates
// the maximal runs of its class, and stage 3 runs inside each PIECE that is left -- a digit group, a run of the CJK class, or the text
// between them.  With E = "a piece starts at this byte" (document and segment starts, digit-group starts, the first byte behind a digit
// run, both ends of a CJK run) stage 3 is local and run-based like the Llama-3 rule (pretok_l3_core.hpp), with E wherever that rule
// reads "a document starts here":
//   * K = \p{L} | \p{M}.  The first char of a K-run starts a match unless the char in front of it (same piece) is its prefix: whitespace
//     that is not CR / LF, or a char no alternative takes (z below), or the ASCII punctuation char of the first alternative.
//   * p = \p{P} | \p{S}.  A p-run is taken whole, with one U+0020 in front of it and the CR / LFs behind it; so the first alternative
//     fires only at a p char that is ASCII, begins its p-run, has no U+0020 in front of it and an ASCII letter behind it.  It takes the
//     ASCII letters that follow and no more: a non-ASCII letter or a mark right behind them starts a match of its own ("!abcé").
//   * whitespace runs exactly as in the Llama-3 rule (l3_space_starts); \s+(?!\S) succeeds at the end of a piece ("a  1" -> a |    | 1).
//   * z = everything else: digits (inside their own pieces), controls, format chars, unassigned.  A z char in front of a K char of its piece is
//     that run's prefix and starts the match; any other z char belongs to a stretch no alternative matches, and Split(Isolated) hands
//     such a stretch on as ONE pre-token: it starts at the first z behind a matched char or a piece edge.
// Every ASCII char that is \p{P} or \p{S} is in the first alternative's class and the other way round (the loader checks the class by its
// member set), so one ASCII mask serves both.  The CJK class is three ranges: a comparison, no table load.
//
// ds3_window_starts is the whole per-lane logic of k_pretok_ds3_lane (kernels/pretok_ds3.hip); ds3_match_piece / ds3_doc_starts are the
// whole per-document logic of k_pretok_ds3_slow.  Both are plain host+device code: tests/test_split_chain.py runs them on the CPU against the
// reference's own pre-tokenizer (tests/harness/ds3_harness.cpp).
#pragma once
#include <cstdint>

#include "pretok_l3_core.hpp"
#include "tables.hpp"

namespace tkamd {

TK_HD bool ds3_is_cjk(uint32_t cp) { return (cp - 0x4E00u) <= (0x9FA5u - 0x4E00u) || (cp - 0x3040u) <= (0x30FFu - 0x3040u); }

// The window's classes arrive in an L3Window: L = ASCII letters, N = ASCII digits, W / R / SP / C / MU as for the Llama-3 rule, AP = ASCII
// punctuation (every ASCII \p{P} or \p{S}); B5 is not read.  uc1 / uc2: the first class table (\p{L}, \p{N}, \s); ps1 / ps2: the second
// (UC2_P, UC2_S, UC2_M).  Returns the pre-token starts of window bytes [8, 56) in bits 8..55 of *start and the bytes it could not decide
// in *unres: a digit or whitespace run that reaches the window's edge (l3_digit_starts, l3_space_starts), and a non-ASCII letter or mark
// behind a run of ASCII letters that reaches the window's first bytes (whether the first alternative took those letters is not known here).
TK_HD void ds3_window_starts(L3Window m, const uint8_t* text, int64_t base, const uint16_t* uc1, const uint8_t* uc2,
                             const uint16_t* ps1, const uint8_t* ps2, uint64_t* start, uint64_t* unres) {
    const uint64_t V = m.V, D = m.D & V, nD = ~D;
    const uint64_t AL = m.L & V, C = m.C & V, SP = m.SP & V, R = m.R & V, PA = m.AP & V;
    uint64_t K = AL, N = m.N, W = m.W, P = PA, J = 0;
    uint64_t U = 0, NM = 0;
    for (uint64_t mm = m.MU & V; mm; mm &= mm - 1) {
        const int k = l3_ctz(mm);
        const uint8_t* p = text + base + k;
        const uint32_t b0 = p[0];
        uint32_t cp, len;
        if (b0 < 0xE0u) { len = 2; cp = ((b0 & 0x1Fu) << 6) | (p[1] & 0x3Fu); }
        else if (b0 < 0xF0u) { len = 3; cp = ((b0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); }
        else { len = 4; cp = ((b0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); }
        const uint32_t f = l3_uc_flags(cp, uc1, uc2);
        const uint64_t span = ((1ull << len) - 1ull) << k;
        if (f & UC_ONIG_L) K |= span;
        else if (f & UC_ONIG_N) { N |= span; NM |= span; }
        else if (f & UC_ONIG_S) W |= span;
        else {
            const uint32_t g = l3_uc_flags(cp, ps1, ps2);
            if (g & UC2_M) K |= span;
            else if (g & (UC2_P | UC2_S)) P |= span;
        }
        if (len == 3 && ds3_is_cjk(cp)) J |= span;
    }
    K &= V; N &= V; W &= V; P &= V; J &= V;
    const uint64_t LEAD = V & ~C;
    const uint64_t X = W | R;
    const uint64_t Z = V & ~(K | P | X);                               // what no alternative takes by itself (digits included: a digit piece holds nothing else)
    // ---- stages 1 and 2: the piece edges
    const uint64_t pN = (N << 1) & nD, pJ = (J << 1) & nD;
    const uint64_t startN = l3_digit_starts(N, NM, LEAD, pN, nD, SPLIT_RULE_LLAMA3, &U);
    const uint64_t E = LEAD & (D | startN | (~N & pN) | (J & ~pJ) | (~J & pJ));
    const uint64_t nE = ~E;
    // ---- stage 3 inside the pieces
    const uint64_t pK = (K << 1) & nE, pW = (W << 1) & nE, pP = (P << 1) & nE, pSP = (SP << 1) & nE, pZ = (Z << 1) & nE;
    const uint64_t startP = P & LEAD & ~(pP | pSP);
    // the first alternative, and the ASCII letters it takes
    const uint64_t A1 = startP & PA & ((AL & nE) >> 1);
    const uint64_t alink = AL & (AL << 1) & nE;                        // bit i: bytes i-1 and i are ASCII letters of one piece
    const uint64_t a1run = l3_spread_fwd((A1 & ~0xFull) << 1, alink);
    // (a letter run from the window's first bytes: its front is not in sight, or the char in front of its punctuation char is not)
    const uint64_t a1unk = l3_spread_fwd((AL & 0xFull) | ((A1 & 0xFull) << 1), alink) & ~a1run;
    const uint64_t Kx = K & LEAD & ~AL;                                // a non-ASCII letter, or a mark
    const uint64_t startK = (K & LEAD & ~(pK | pW | pZ | (A1 << 1))) | (Kx & (a1run << 1) & nE);
    U |= Kx & (a1unk << 1) & nE;
    // a z char is its stretch's first one, or the prefix of the K-run behind it
    uint64_t Yk = (K & LEAD & nE) >> 1;
    Yk |= (Yk & C) >> 1; Yk |= (Yk & C) >> 1; Yk |= (Yk & C) >> 1;
    const uint64_t startZ = Z & LEAD & (~pZ | Yk);
    uint64_t tailA;
    const uint64_t startX = l3_space_starts(X, W, R, C, LEAD, E, pP, &U, &tailA);
    (void)tailA;
    *start = LEAD & (E | startK | startP | startZ | startX) & L3W_MAIN_MASK;
    *unres = U & L3W_MAIN_MASK;
}

// ASCII flag entry of one byte value for the caller's 256-entry table, in l3_byte_flags' layout: bits 0 / 8 / 16 / 24 of .x = ASCII letter,
// ASCII digit, whitespace except CR / LF, CR / LF; of .y = U+0020, continuation byte, ASCII punctuation, multi-byte lead
TK_HD L3Flags ds3_byte_flags(uint32_t v) {
    L3Flags f = l3_byte_flags(v);
    const bool isP = v > 0x20u && v < 0x7Fu && !(f.x & 0x101u);
    f.y = (f.y & ~(1u << 16)) | (isP ? 1u << 16 : 0u);
    return f;
}

// ---- the sequential matcher: exact for any run length ------------------------------------------------------------------------------
struct Ds3Seq {
    const uint16_t* uc1;
    const uint8_t* uc2;
    const uint16_t* ps1;
    const uint8_t* ps2;
};
enum : uint32_t { DS3_Z = 0, DS3_K = 1, DS3_P = 2, DS3_W = 3, DS3_R = 4, DS3_N = 8, DS3_J = 16, DS3_CLS = 7 };
TK_HD uint32_t ds3_dec(const uint8_t* s, int64_t i, int64_t n, int* len) {
    const uint32_t b = s[i];
    if (b < 0x80u) { *len = 1; return b; }
    if (b >= 0xC0u && b < 0xE0u && i + 1 < n) { *len = 2; return ((b & 0x1Fu) << 6) | (s[i + 1] & 0x3Fu); }
    if (b >= 0xE0u && b < 0xF0u && i + 2 < n) { *len = 3; return ((b & 0x0Fu) << 12) | ((s[i + 1] & 0x3Fu) << 6) | (s[i + 2] & 0x3Fu); }
    if (b >= 0xF0u && i + 3 < n) { *len = 4; return ((b & 0x07u) << 18) | ((s[i + 1] & 0x3Fu) << 12) | ((s[i + 2] & 0x3Fu) << 6) | (s[i + 3] & 0x3Fu); }
    *len = 1;
    return 0xFFFDu;
}
// class of one code point: DS3_Z / K / P / W / R, with DS3_N on a digit and DS3_J on a char of the CJK class
TK_HD uint32_t ds3_cls(const Ds3Seq& q, uint32_t cp) {
    if (cp == '\r' || cp == '\n') return DS3_R;
    const uint32_t j = ds3_is_cjk(cp) ? DS3_J : 0u;
    const uint32_t f = l3_uc_flags(cp, q.uc1, q.uc2);
    if (f & UC_ONIG_L) return DS3_K | j;
    if (f & UC_ONIG_N) return DS3_Z | DS3_N;
    if (f & UC_ONIG_S) return DS3_W;
    const uint32_t g = l3_uc_flags(cp, q.ps1, q.ps2);
    if (g & UC2_M) return DS3_K | j;
    if (g & (UC2_P | UC2_S)) return DS3_P | j;
    return DS3_Z | j;
}
TK_HD bool ds3_ascii_letter(uint32_t b) { return ((b | 0x20u) - 'a') < 26u; }
// One leftmost-first match of the third Split's pattern at s[i] inside the piece that ends at n (the alternatives in the pattern's order,
// each with the backtracking the regex engine would do); returns its end, or i when no alternative matches there
TK_HD int64_t ds3_match_piece(const Ds3Seq& q, const uint8_t* s, int64_t i, int64_t n) {
    int l;
    const uint32_t c = ds3_dec(s, i, n, &l);
    const uint32_t cc = ds3_cls(q, c) & DS3_CLS;
    if (cc == DS3_P && c < 0x80u && i + 1 < n && ds3_ascii_letter(s[i + 1])) {          // [ASCII punctuation][A-Za-z]+
        int64_t j = i + 2;
        while (j < n && ds3_ascii_letter(s[j])) ++j;
        return j;
    }
    {   // [^\r\n\p{L}\p{P}\p{S}]?[\p{L}\p{M}]+
        int64_t k = -1;
        if (cc == DS3_K) k = i;
        else if (cc != DS3_R && cc != DS3_P && i + l < n) {
            int lk;
            if ((ds3_cls(q, ds3_dec(s, i + l, n, &lk)) & DS3_CLS) == DS3_K) k = i + l;
        }
        if (k >= 0) {
            int64_t j = k;
            while (j < n) { int lj; if ((ds3_cls(q, ds3_dec(s, j, n, &lj)) & DS3_CLS) != DS3_K) break; j += lj; }
            return j;
        }
    }
    {   // " ?[\p{P}\p{S}]+[\r\n]*"
        const int64_t k = (c == ' ') ? i + 1 : i;
        if (k < n) {
            int lk;
            if ((ds3_cls(q, ds3_dec(s, k, n, &lk)) & DS3_CLS) == DS3_P) {
                int64_t j = k + lk;
                while (j < n) { int lj; if ((ds3_cls(q, ds3_dec(s, j, n, &lj)) & DS3_CLS) != DS3_P) break; j += lj; }
                while (j < n && (s[j] == '\r' || s[j] == '\n')) ++j;
                return j;
            }
        }
    }
    if (cc >= DS3_W) {
        int64_t j = i, last = -1, cur = i;
        while (j < n) { int lj; const uint32_t k = ds3_cls(q, ds3_dec(s, j, n, &lj)) & DS3_CLS; if (k < DS3_W) break; if (k == DS3_R) last = j; cur = j; j += lj; }
        if (last >= 0) return last + 1;          // \s*[\r\n]+
        if (j >= n) return j;                    // \s+(?!\S) at the end of the piece
        if (cur > i) return cur;                 // \s+(?!\S): all but the last whitespace char
        return j;                                // \s+
    }
    return i;
}
// Every pre-token start of the document s[0, n), in order, handed to emit(byte): the pieces of stages 1 and 2, then stage 3 inside each
template <class Emit>
TK_HD void ds3_doc_starts(const Ds3Seq& q, const uint8_t* s, int64_t n, Emit emit) {
    int64_t i = 0;
    while (i < n) {
        int l;
        const uint32_t c0 = ds3_cls(q, ds3_dec(s, i, n, &l));
        int64_t e = i + l;
        if (c0 & DS3_N) {
            for (int cnt = 1; cnt < 3 && e < n; ++cnt) { int lj; if (!(ds3_cls(q, ds3_dec(s, e, n, &lj)) & DS3_N)) break; e += lj; }
        } else {
            const uint32_t j0 = c0 & DS3_J;
            while (e < n) { int lj; const uint32_t cj = ds3_cls(q, ds3_dec(s, e, n, &lj)); if ((cj & DS3_N) || (cj & DS3_J) != j0) break; e += lj; }
        }
        bool gap = false;                        // inside a stretch no alternative matches: one pre-token
        int64_t p = i;
        while (p < e) {
            const int64_t m = ds3_match_piece(q, s, p, e);
            if (m > p) { emit(p); p = m; gap = false; }
            else {
                if (!gap) emit(p);
                gap = true;
                int lp;
                ds3_dec(s, p, e, &lp);
                p += lp;
            }
        }
        i = e;
    }
}

}  // namespace tkamd
