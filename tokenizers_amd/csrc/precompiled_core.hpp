// The Precompiled normalizer (normalizers/precompiled.rs over the spm_precompiled crate: SentencePiece's precompiled_charsmap), one
// host+device core: the probe of the charsmap's double-array trie, the extended grapheme cluster rule (UAX #29) the reference cuts a
// piece with, and what one char of the text becomes.  kernels/precompiled.hip runs it per lane; HostModel::precompiled_normalize runs
// it for the load-time probe and for tests/harness/precompiled_harness.cpp, which holds it against the reference wheel.
//
// The blob: u32 LE trie_bytes, trie_bytes / 4 little-endian u32 units of a darts-clone double array, then NUL-terminated replacement
// strings.  common_prefix_search walks the key's bytes -- pos ^= offset(unit[pos]) at the root, then per byte c: pos ^= c, the unit
// there must carry the label c, pos ^= its offset, and a unit with has_leaf has its value (an offset into the replacement strings)
// in the unit at pos -- and the reference takes the FIRST result: the shortest key that is a prefix.  The reference panics when pos
// leaves the array; here an index outside it is "no match", and the loader refuses a blob whose reachable units point outside.
//
// normalize: the piece is cut into extended grapheme clusters; a cluster of fewer than 6 bytes is looked up whole and on a hit the
// replacement stands for all of it; otherwise every char of it is looked up alone, replaced on a hit and copied on a miss.  So what a
// char becomes is a function of the char and of its cluster alone (pc_char_out): every lane works it out for the chars whose first
// byte it holds, no lane waits for another.
//
// Alignment (precompiled.rs replace() -> NormalizedString::transform): the i-th char of a replacement takes the i-th source char of
// what it replaces, the chars beyond the last source char that one; source chars beyond the replacement's are consumed by the output
// char in front of them -- or, when that char is an inserted one, re-align it to the first of them (pc_tail_moves).  One source char per output char, so one `norig` entry per output byte serves.  The one exception is
// sequential: a replacement by NOTHING at the very start of a piece (U+FEFF in front of a document) has no output char in front of it,
// the reference loses those source chars, and every later char of the piece is aligned that many source chars too early --
// pc_lost_chars counts them, kernels/precompiled.hip k_pc_lost_fix moves the piece's entries.
#pragma once
#include <cstdint>

#include "nfc_core.hpp"

namespace tkamd {

constexpr uint32_t GC_OTHER = 0, GC_CR = 1, GC_LF = 2, GC_CONTROL = 3, GC_EXTEND = 4, GC_ZWJ = 5, GC_RI = 6, GC_PREPEND = 7, GC_SPACING = 8, GC_L = 9, GC_V = 10,
                   GC_T = 11, GC_LV = 12, GC_LVT = 13, GC_MASK = 15, GC_EXTPICT = 16, GC_INCB_SHIFT = 5, GC_INCB_CONSONANT = 1, GC_INCB_EXTEND = 2, GC_INCB_LINKER = 3;
constexpr int PC_LANE = 16;                 // source bytes a lane of the kernels takes
constexpr uint32_t PC_WHOLE_MAX = 6;        // a cluster of fewer bytes is looked up whole first
constexpr uint32_t PC_REP_MAX = 255;        // bytes of one replacement (the count pass keeps a byte per source byte); longer ones are refused at load

struct PcTables {
    const uint32_t* units;                  // the double array
    uint32_t n_units;
    const uint8_t* rep;                     // the replacement strings, n_rep bytes, the last one a NUL (checked at load)
    uint32_t n_rep;
    const uint16_t* g1;                     // grapheme classes (grapheme_tables.inc), two stages
    const uint8_t* g2;
    unsigned long long first[4];            // byte b starts a key
};

TK_HD uint32_t pc_class(const PcTables& t, uint32_t cp) {
    if (cp - 0xAC00u < 11172u) return (cp - 0xAC00u) % 28u == 0u ? GC_LV : GC_LVT;
    return cp >= 0x110000u ? 0u : t.g2[((uint32_t)t.g1[cp >> 8] << 8) | (cp & 255u)];
}
TK_HD bool pc_first(const PcTables& t, uint32_t b) { return ((t.first[b >> 6] >> (b & 63u)) & 1ull) != 0; }

// the first result of common_prefix_search over key[0, len): *ro / *rl = where its replacement lies in t.rep
TK_HD bool pc_lookup(const PcTables& t, const uint8_t* key, uint32_t len, uint32_t* ro, uint32_t* rl) {
    if (t.n_units == 0u) return false;
    uint32_t u = t.units[0];
    uint32_t pos = (u >> 10) << ((u & 0x200u) >> 6);
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t c = key[k];
        if (c == 0u) return false;
        pos ^= c;
        if (pos >= t.n_units) return false;
        u = t.units[pos];
        if ((u & 0x800000FFu) != c) return false;
        pos ^= (u >> 10) << ((u & 0x200u) >> 6);
        if ((u >> 8) & 1u) {
            if (pos >= t.n_units) return false;
            const uint32_t v = t.units[pos] & 0x7FFFFFFFu;
            if (v >= t.n_rep) return false;
            uint32_t e = v;
            while (e < t.n_rep && t.rep[e] != 0u) ++e;
            *ro = v;
            *rl = e - v;
            return true;
        }
    }
    return false;
}

// a piece starts at p: the text's first byte, a document start, either edge of a verbatim added-token match (the bound mask)
TK_HD bool pc_piece_start(const nfc_mask_t* bound, int64_t p) { return p <= 0 || nfc_bit(bound, p); }

// Is there a cluster boundary in front of the char that starts at p?  (GB1-GB999; the three rules that look further back than the char
// in front: GB9c and GB11 walk back over the run of Extend / Linker chars in front of p, never across a piece start -- once per char that
// ENDS such a run, so linear in the text; GB12/13 need no walk, see below.)
TK_HD bool pc_boundary(const PcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t p) {
    if (p >= n || pc_piece_start(bound, p)) return true;
    uint32_t l;
    const int64_t q = nfc_unit_start(text, n, p - 1);
    const uint32_t bb = text[p], ab = text[q];
    if ((ab | bb) < 0x80u) return !(ab == 13u && bb == 10u);         // ASCII: Other / Control / CR / LF, only CR x LF holds together
    const uint32_t B = pc_class(t, nfc_decode(text, n, p, &l)), A = pc_class(t, nfc_decode(text, n, q, &l));
    const uint32_t a = A & GC_MASK, b = B & GC_MASK;
    if (a == GC_CR && b == GC_LF) return false;                                                  // GB3
    if (a == GC_CR || a == GC_LF || a == GC_CONTROL) return true;                                // GB4
    if (b == GC_CR || b == GC_LF || b == GC_CONTROL) return true;                                // GB5
    if (a == GC_L && (b == GC_L || b == GC_V || b == GC_LV || b == GC_LVT)) return false;        // GB6
    if ((a == GC_LV || a == GC_V) && (b == GC_V || b == GC_T)) return false;                     // GB7
    if ((a == GC_LVT || a == GC_T) && b == GC_T) return false;                                   // GB8
    if (b == GC_EXTEND || b == GC_ZWJ || b == GC_SPACING) return false;                          // GB9, GB9a
    if (a == GC_PREPEND) return false;                                                           // GB9b
    const uint32_t ia = A >> GC_INCB_SHIFT, ib = B >> GC_INCB_SHIFT;
    if (ib == GC_INCB_CONSONANT && (ia == GC_INCB_EXTEND || ia == GC_INCB_LINKER)) {             // GB9c
        bool linker = false;
        for (int64_t r = q;;) {
            const uint32_t ir = pc_class(t, nfc_decode(text, n, r, &l)) >> GC_INCB_SHIFT;
            if (ir == GC_INCB_LINKER) linker = true;
            else if (ir != GC_INCB_EXTEND) { if (ir == GC_INCB_CONSONANT && linker) return false; break; }
            if (pc_piece_start(bound, r)) break;
            r = nfc_unit_start(text, n, r - 1);
        }
    }
    if (a == GC_ZWJ && (B & GC_EXTPICT)) {                                                       // GB11
        for (int64_t r = q; !pc_piece_start(bound, r);) {
            r = nfc_unit_start(text, n, r - 1);
            const uint32_t R = pc_class(t, nfc_decode(text, n, r, &l));
            if ((R & GC_MASK) == GC_EXTEND) continue;
            if (R & GC_EXTPICT) return false;
            break;
        }
    }
    // GB12, GB13: whether two regional indicators pair depends on the parity of the run in front.  Nothing here can tell the difference
    // -- an indicator is 4 bytes, so a cluster of two is never looked up whole and one alone is its own char either way -- and a walk
    // over the run for every one of its chars would be quadratic: the run holds together.
    if (a == GC_RI && b == GC_RI) return false;
    return true;
}

// What the char whose first byte is text[p] becomes.  PC_COPY: itself.  PC_NONE: nothing (its cluster's first char stands for it).
// PC_REP: the replacement t.rep[*ro, *ro + *rl) of the source chars text[p, *se) -- the whole cluster, or the char alone.
enum PcOut { PC_COPY = 0, PC_NONE = 1, PC_REP = 2 };
TK_HD PcOut pc_char_out(const PcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t p, uint32_t* ro, uint32_t* rl, int64_t* se) {
    uint32_t l;
    nfc_decode(text, n, p, &l);
    const bool head = pc_boundary(t, text, n, bound, p);
    // (the usual char: it opens a cluster and no key starts with its first byte -- neither the cluster nor the char can hit)
    if (head && !pc_first(t, text[p])) return PC_COPY;
    // (back to the cluster's first char, but no further than a cluster that is looked up whole can reach: at most five bytes)
    int64_t s = p;
    while ((uint32_t)(p + l - s) < PC_WHOLE_MAX && !pc_boundary(t, text, n, bound, s)) s = nfc_unit_start(text, n, s - 1);
    if ((uint32_t)(p + l - s) < PC_WHOLE_MAX && pc_first(t, text[s])) {
        int64_t e = p + l;
        while ((uint32_t)(e - s) < PC_WHOLE_MAX && !pc_boundary(t, text, n, bound, e)) { uint32_t le; nfc_decode(text, n, e, &le); e += le; }
        if ((uint32_t)(e - s) < PC_WHOLE_MAX && pc_boundary(t, text, n, bound, e) && pc_lookup(t, text + s, (uint32_t)(e - s), ro, rl)) {
            *se = e;
            return s == p ? PC_REP : PC_NONE;
        }
    }
    if (pc_first(t, text[p]) && pc_lookup(t, text + p, l, ro, rl)) { *se = p + l; return PC_REP; }
    return PC_COPY;
}

// A replacement with more chars than it replaces ends in INSERTED chars; when what follows it in the piece (at se) becomes nothing, the
// reference charges those source chars to the last entry of its list -- that inserted char, which so turns into one aligned to the
// first of them ("ﬃ\x1e": the i of f f i sits on the \x1e).  True: the replacement's last char takes the source char at se.
TK_HD bool pc_tail_moves(const PcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t se) {
    if (se >= n || nfc_bit(bound, se)) return false;
    uint32_t ro, rl = 1u;
    int64_t e;
    return pc_char_out(t, text, n, bound, se, &ro, &rl, &e) == PC_REP && rl == 0u;
}

// The source chars the reference loses at the start of the piece that starts at p (not a verbatim byte): those of the clusters in
// front of the piece's first output char -- every one of them became nothing, alone or with its cluster.
TK_HD uint32_t pc_lost_chars(const PcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t p) {
    uint32_t lost = 0u, l, ro, rl;
    int64_t se;
    while (p < n) {
        const PcOut k = pc_char_out(t, text, n, bound, p, &ro, &rl, &se);
        if (k == PC_COPY || (k == PC_REP && rl != 0u)) break;
        nfc_decode(text, n, p, &l);
        p += l;
        ++lost;
        if (p < n && nfc_bit(bound, p)) break;
    }
    return lost;
}

// the start of the char `back` chars in front of the one that starts at p
TK_HD int64_t pc_chars_back(const uint8_t* text, int64_t n, int64_t p, uint32_t back) {
    while (back-- && p > 0) p = nfc_unit_start(text, n, p - 1);
    return p;
}

}  // namespace tkamd
