// The NFC normalizer (normalizers/unicode.rs NFC -> tokenizer/normalizer.rs:461-464 -> unicode-normalization-alignments), one host+device
// core: the quick check, the segment rules, and the normalization of one segment with the alignment NormalizedString::transform
// (tokenizer/normalizer.rs:317-428) gives every output char.  kernels/nfc.hip runs it per lane; the loader normalizes the patterns of
// normalized added tokens with it; tests/harness/nfc_harness.cpp holds it against the reference wheel.
//
// Data (nfc_tables.inc, probed from the wheel): one byte per code point in a 2-stage table -- the rank of its canonical combining class
// among the classes in use (the order is all that ordering and blocking ask of a class), DECOMPOSES, and "NFC_Quick_Check is not Yes" --
// and one pair table holding the full canonical decompositions (keys (cp, 0): three code points, (cp, 1): the fourth) next to the primary
// composites (keys (first, second): a second is never below U+0300, so the two kinds of key never meet).  Hangul is arithmetic.
//
// A char is ACTIVE when its class is not 0 or its quick check is not Yes: only such a char can change, move, or compose with what
// stands in front of it.  A SEGMENT starts at a char that is not active, or at a piece start (a document start, either edge of a
// verbatim added-token match), and runs through every active char behind it.  Segments are independent: a char that is not active is a
// starter that composes with nothing in front of it, so neither the ordering nor the composition crosses it.  A segment of one char that
// is not active is the char itself (TRIVIAL); every other one is decomposed, stable-sorted by class, and composed with the blocking rule.
//
// Alignment.  The reference's iterators yield (char, change): a decomposition's first char 0, its further chars 1; a composition of k
// and c carries k's change + c's change - 1; the pairs move through the canonical ordering together.  transform() then walks the SOURCE
// chars by position: a char with change <= 0 takes the alignment of the next source char and consumes it and -change more; a char with
// change > 0 takes the alignment of the source char consumed last.  Every output char is so aligned to exactly ONE source char, which is
// why one `norig` entry per output byte (the source char's first byte) is all the offsets need.
#pragma once
#include <cstdint>

#include "tables.hpp"
#include "nfkc_tables.inc"          // (no NFKC_WANT_*: the generator's figures only -- NFKC_GROWTH, NFKC_MAX_DECOMP)

namespace tkamd {

#if defined(__HIPCC__)
#define TK_HD_OUTLINE inline __host__ __device__ __attribute__((noinline))
#else
#define TK_HD_OUTLINE inline
#endif

constexpr uint32_t NFC_F_RANK = 0x3Fu, NFC_F_DECOMP = 0x40u, NFC_F_QCN = 0x80u, NFC_F_ACTIVE = NFC_F_RANK | NFC_F_QCN;
constexpr int NFC_SEG_MAX = 48;        // pieces (and source chars) of one segment, like BN_RUN_MAX; a longer one refuses the batch
constexpr int NFC_LANE = 16;           // source bytes a lane of the kernels takes (= BN_LANE: the BnOlen layout)
constexpr uint32_t NFC_S_BASE = 0xAC00u, NFC_L_BASE = 0x1100u, NFC_V_BASE = 0x1161u, NFC_T_BASE = 0x11A7u, NFC_V_N = 21u, NFC_T_N = 28u,
                   NFC_S_N = 19u * 21u * 28u;
constexpr uint32_t NFC_FILL = 0x1FFFFFu;

// NFD mode (a normalizer chain of NFD and Lowercase with no StripAccents, tables.hpp NORM_CHAIN): the same segments, decomposed and
// ordered but not composed; Lowercase, a map of single chars, is applied to every source char in front of its decomposition
// (Sequence[Lowercase, NFD]: a char it makes two of is two source chars to NFD, both aligned to the one) or to every piece behind the
// ordering (Sequence[NFD, Lowercase]: one char each there -- the one char to_lowercase makes two of, U+0130, decomposes first).
constexpr uint32_t NFD_MODE = 1u, NFD_LOWER_FIRST = 2u, NFD_LOWER_LAST = 4u, NFD_LOWER = NFD_LOWER_FIRST | NFD_LOWER_LAST;
// NFC_LOWER (Sequence[NFC, Lowercase] of the CLIP files, tables.hpp NORM_NFC_LOWER): the segments of NFC, composed as NFC composes them,
// and to_lowercase -- the same tables, in the same slots -- applied to every char of the composed segment.  What it makes of one char
// (two of U+0130) is aligned to the source char that char was aligned to.  A char that lowercases changes on its own, like one that
// decomposes in NFD mode: it is no trivial segment, no plain lane (but for all-ASCII lanes, lowercased on the copy), and the quick
// check does not vouch for it.
constexpr uint32_t NFC_LOWER = 8u, NFC_ANY_LOWER = NFD_LOWER | NFC_LOWER;

// K mode (NFKC, tables.hpp NORM_NFKC): a COMPILE-TIME mode -- template <bool K> below; NFC and NFD are the K = false instantiations and
// read none of this.  The flags n1 / n2 are then those of nfkc_tables.inc (the same ranks, K-DECOMPOSES, "NFKC_Quick_Check is not Yes"),
// the decompositions are the full compatibility ones, of up to NFKC_MAX_DECOMP code points: lmap (cp, 0) -> (offset, length) into
// kflat.  The primary composites stay NFC's own (map).  A decomposition's first char has change 0 and every further one 1, as before
// ("\uFB01" -> "fi", both aligned to the one source char).
// The head rule is wider in K mode: thousands of chars change under NFKC on their own (every fullwidth letter, U+3000, the ligatures),
// all ACTIVE by their quick check, and a run of them would be one segment.  There a char ALSO opens a segment when its full
// decomposition begins with a char that is not active -- class 0, no second of a primary composite, no Hangul V / T.  That is exact:
// such a first char is a starter that composes with nothing in front of it, so what NFKC makes of the text in front ends before it,
// and neither the ordering nor the composition crosses it -- NFKC(p + c + s) = NFKC(p) + NFKC(c + s).
constexpr uint32_t NFK_GROWTH = NFKC_GROWTH;      // UTF-8 bytes a source byte can stand for (U+FDFA: 3 -> 33)

struct NfcTables {
    const uint16_t* n1;
    const uint8_t* n2;
    const MergeSlot* map;
    uint32_t map_mask, map_seed;
    uint32_t mode = 0u;                  // 0: NFC
    // NFD_LOWER_*: to_lowercase in the BertNormalizer's layout -- flag 1 on every char it changes, (cp, 0) -> up to three code points
    // (K mode, which never lowercases, keeps its tables in these slots -- kflat in l1's, its pair table as lmap / lmap_mask / lmap_seed --:
    // the struct is copied into the scratch of every lane that calls the outlined routines, and NFC's and NFD's must not grow for a mode they never run)
    union {
        const uint16_t* l1 = nullptr;
        const uint32_t* kflat;           // K mode: the full compatibility decompositions, one after the other
    };
    const uint8_t* l2 = nullptr;
    const MergeSlot* lmap = nullptr;
    uint32_t lmap_mask = 0u, lmap_seed = 0u;
};
using nfc_mask_t = unsigned long long;

TK_HD uint32_t nfc_flags(const NfcTables& t, uint32_t cp) { return cp >= 0x110000u ? 0u : t.n2[((uint32_t)t.n1[cp >> 8] << 8) | (cp & 255u)]; }
TK_HD bool nfc_bit(const nfc_mask_t* m, int64_t i) { return ((m[i >> 6] >> (i & 63)) & 1ull) != 0; }
TK_HD bool nfc_map(const NfcTables& t, uint32_t a, uint32_t b, uint32_t* lo, uint32_t* hi) {
    const MergeSlot& x = t.map[merge_hash1(a, b, t.map_seed) & t.map_mask];
    const MergeSlot& y = t.map[merge_hash2(a, b, t.map_seed) & t.map_mask];
    const MergeSlot* h = (x.a == a && x.b == b) ? &x : (y.a == a && y.b == b) ? &y : nullptr;
    if (!h) return false;
    *lo = h->rank;
    *hi = h->new_id;
    return true;
}
// K mode: the full compatibility decomposition of cp, kflat[*off .. *off + *len)
TK_HD bool nfk_map(const NfcTables& t, uint32_t cp, uint32_t* off, uint32_t* len) {
    const MergeSlot& x = t.lmap[merge_hash1(cp, 0u, t.lmap_seed) & t.lmap_mask];
    const MergeSlot& y = t.lmap[merge_hash2(cp, 0u, t.lmap_seed) & t.lmap_mask];
    const MergeSlot* h = (x.a == cp && x.b == 0u) ? &x : (y.a == cp && y.b == 0u) ? &y : nullptr;
    if (!h) return false;
    *off = h->rank;
    *len = h->new_id;
    return true;
}
// does the char (flags f) open a segment wherever it stands?  One that is not active; in K mode also one whose decomposition begins with such a char
template <bool K = false>
TK_HD bool nfc_head(const NfcTables& t, uint32_t cp, uint32_t f) {
    if (!(f & NFC_F_ACTIVE)) return true;
    if constexpr (K) {
        uint32_t off, len;
        if ((f & NFC_F_DECOMP) && nfk_map(t, cp, &off, &len)) return !(nfc_flags(t, t.kflat[off]) & NFC_F_ACTIVE);
    }
    return false;
}
TK_HD bool nfd_lowercases(const NfcTables& t, uint32_t cp) { return cp < 0x110000u && (t.l2[((uint32_t)t.l1[cp >> 8] << 8) | (cp & 255u)] & 1u) != 0u; }
// to_lowercase of cp: out[0 .. returned) (the char itself where it has none)
TK_HD int nfd_lower(const NfcTables& t, uint32_t cp, uint32_t* out) {
    out[0] = cp;
    if (!nfd_lowercases(t, cp)) return 1;
    const MergeSlot& x = t.lmap[merge_hash1(cp, 0u, t.lmap_seed) & t.lmap_mask];
    const MergeSlot& y = t.lmap[merge_hash2(cp, 0u, t.lmap_seed) & t.lmap_mask];
    const MergeSlot* h = (x.a == cp && x.b == 0u) ? &x : (y.a == cp && y.b == 0u) ? &y : nullptr;
    if (!h) return 1;
    const unsigned long long v = ((unsigned long long)h->new_id << 32) | h->rank;
    int k = 0;
    for (int q = 0; q < 3; ++q) {
        const uint32_t c = (uint32_t)((v >> (21 * q)) & 0x1FFFFFu);
        if (c != 0x1FFFFFu) out[k++] = c;
    }
    return k;
}
// NFD mode: does the char (flags f) change on its own -- a decomposition, a lowercase form?
// (NFC_LOWER: a lowercase form alone -- a char that decomposes and composes again is NFC as it stands)
TK_HD bool nfd_changes(const NfcTables& t, uint32_t cp, uint32_t f) {
    return ((t.mode & NFD_MODE) && (f & 0x40u) != 0u) || ((t.mode & NFC_ANY_LOWER) && nfd_lowercases(t, cp));
}
TK_HD uint32_t nfc_utf8_len(uint32_t cp) { return cp < 0x80u ? 1u : cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u; }
TK_HD uint32_t nfc_utf8_put(uint8_t* o, uint32_t c) {
    if (c < 0x80u) { o[0] = (uint8_t)c; return 1u; }
    if (c < 0x800u) { o[0] = (uint8_t)(0xC0u | (c >> 6)); o[1] = (uint8_t)(0x80u | (c & 0x3Fu)); return 2u; }
    if (c < 0x10000u) { o[0] = (uint8_t)(0xE0u | (c >> 12)); o[1] = (uint8_t)(0x80u | ((c >> 6) & 0x3Fu)); o[2] = (uint8_t)(0x80u | (c & 0x3Fu)); return 3u; }
    o[0] = (uint8_t)(0xF0u | (c >> 18)); o[1] = (uint8_t)(0x80u | ((c >> 12) & 0x3Fu)); o[2] = (uint8_t)(0x80u | ((c >> 6) & 0x3Fu)); o[3] = (uint8_t)(0x80u | (c & 0x3Fu));
    return 4u;
}

// The unit whose first byte is text[i] (i < n): a lead byte with all its continuation bytes inside the text is the code point; any
// other byte -- ASCII, a stray continuation byte, a lead byte cut short -- is a unit of one byte (U+FFFD for the last two: not active).
TK_HD uint32_t nfc_decode(const uint8_t* text, int64_t n, int64_t i, uint32_t* len) {
    const uint32_t b0 = text[i];
    *len = 1u;
    if (b0 < 0x80u) return b0;
    if (b0 < 0xC0u) return 0xFFFDu;
    const uint32_t l = b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : 4u;
    if (i + (int64_t)l > n) return 0xFFFDu;
    uint32_t cp = b0 & (0xFFu >> (l + 1u));
    for (uint32_t k = 1; k < l; ++k) {
        const uint32_t c = text[i + k];
        if ((c & 0xC0u) != 0x80u) return 0xFFFDu;
        cp = (cp << 6) | (c & 0x3Fu);
    }
    *len = l;
    return cp;
}
// first byte of the unit that holds byte j
TK_HD int64_t nfc_unit_start(const uint8_t* text, int64_t n, int64_t j) {
    if ((text[j] & 0xC0u) != 0x80u) return j;
    for (int64_t k = 1; k <= 3 && j - k >= 0; ++k) {
        const uint32_t c = text[j - k];
        if ((c & 0xC0u) == 0x80u) continue;
        if (c >= 0xC0u) {
            uint32_t l;
            nfc_decode(text, n, j - k, &l);
            if ((int64_t)l > k) return j - k;
        }
        break;
    }
    return j;
}

// ---- the quick check of one 16-byte lane (k_nfc_check): true = "not known to be NFC".  Exact in the direction that matters: a text
// every lane of which passes has all chars Quick_Check = Yes and every run of non-starters in class order, so it IS its NFC form, and so
// is every piece of it (pieces are ignored here: a mark that opens a piece is held against the char in front of it all the same, the one
// place where an NFC text can fail the check).
TK_HD bool nfc_check_lane(const NfcTables& t, const uint8_t* text, int64_t n, int64_t i0) {
    uint32_t prev = 0xFFFFFFFFu;                            // class rank of the char in front (not looked up yet)
    const int64_t i1 = i0 + NFC_LANE < n ? i0 + NFC_LANE : n;
    for (int64_t i = i0; i < i1; ++i) {
        const uint32_t b = text[i];
        if (b < 0x80u) {
            if ((t.mode & NFC_LOWER) && b - 0x41u < 26u) return true;
            prev = 0u;
            continue;
        }
        if (b < 0xC0u) continue;
        uint32_t l;
        const uint32_t cp = nfc_decode(text, n, i, &l), f = nfc_flags(t, cp);
        if (f & NFC_F_QCN) return true;
        if ((t.mode & NFC_LOWER) && nfd_lowercases(t, cp)) return true;
        const uint32_t r = f & NFC_F_RANK;
        if (r) {
            if (prev == 0xFFFFFFFFu) {
                prev = 0u;
                if (i > 0) {
                    uint32_t pl;
                    prev = nfc_flags(t, nfc_decode(text, n, nfc_unit_start(text, n, i - 1), &pl)) & NFC_F_RANK;
                }
            }
            if (prev > r) return true;
        }
        prev = r;
    }
    return false;
}

// ---- segments
// first byte of the segment that holds the unit starting at cs, or -1 if more than NFC_SEG_MAX chars lie between them
template <bool K = false>
TK_HD int64_t nfc_seg_start(const NfcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t cs) {
    int64_t s = cs;
    for (int steps = 0; steps <= NFC_SEG_MAX; ++steps) {
        if (s <= 0 || nfc_bit(bound, s)) return s;
        uint32_t l;
        const uint32_t cp = nfc_decode(text, n, s, &l);
        if (nfc_head<K>(t, cp, nfc_flags(t, cp))) return s;
        s = nfc_unit_start(text, n, s - 1);
    }
    return -1;
}
// the unit at s (flags f, length l) is a segment head: is the segment that unit alone, unchanged?
template <bool K = false>
TK_HD bool nfc_trivial(const NfcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t s, uint32_t f, uint32_t l) {
    if (f & NFC_F_ACTIVE) return false;
    if (t.mode) {                                           // (NFD mode: a char that decomposes or lowercases is a segment to normalize)
        uint32_t l0;
        if (nfd_changes(t, nfc_decode(text, n, s, &l0), f)) return false;
    }
    const int64_t p = s + l;
    if (p >= n || nfc_bit(bound, p)) return true;
    if (text[p] < 0x80u) return true;
    uint32_t l2;
    const uint32_t c2 = nfc_decode(text, n, p, &l2);
    return nfc_head<K>(t, c2, nfc_flags(t, c2));
}
// output bytes charged to source byte k of a segment of S source bytes and O output bytes (O <= 3 S): one each as far as they go, then
// up to two more each from the front.  A segment that keeps its length charges every byte 1, as a lane that is copied whole does.
TK_HD uint32_t nfc_charge(uint32_t k, uint32_t O, uint32_t S) {
    const uint32_t base = O < S ? O : S, extra = O - base;
    const uint32_t x = extra > 2u * k ? extra - 2u * k : 0u;
    return (k < O ? 1u : 0u) + (x > 2u ? 2u : x);
}

// the same for a growth of G a byte (K mode: NFK_GROWTH): one each as far as they go, then up to G - 1 more each from the front
template <uint32_t G>
TK_HD uint32_t nfc_charge_g(uint32_t k, uint32_t O, uint32_t S) {
    const uint32_t base = O < S ? O : S, extra = O - base;
    const uint32_t x = extra > (G - 1u) * k ? extra - (G - 1u) * k : 0u;
    return (k < O ? 1u : 0u) + (x > G - 1u ? G - 1u : x);
}

struct NfcSeg {
    uint32_t cp[NFC_SEG_MAX];          // pieces, then the output chars
    uint8_t rank[NFC_SEG_MAX];
    int8_t chg[NFC_SEG_MAX];
    uint8_t src[NFC_SEG_MAX];          // first byte of every source char, relative to the segment's
    uint8_t al[NFC_SEG_MAX];           // per output char: first byte of the source char it is aligned to, relative to the segment's
    int n;                             // output chars
    int64_t e;                         // end of the segment in the text
    uint32_t obytes;                   // UTF-8 bytes of the output
};

TK_HD uint32_t nfc_compose(const NfcTables& t, uint32_t a, uint32_t b) {
    if (a - NFC_L_BASE < 19u && b - NFC_V_BASE < NFC_V_N) return NFC_S_BASE + ((a - NFC_L_BASE) * NFC_V_N + (b - NFC_V_BASE)) * NFC_T_N;
    if (a - NFC_S_BASE < NFC_S_N && (a - NFC_S_BASE) % NFC_T_N == 0u && b - (NFC_T_BASE + 1u) < NFC_T_N - 1u) return a + (b - NFC_T_BASE);
    if (b < 0x300u) return 0u;
    uint32_t lo, hi;
    return nfc_map(t, a, b, &lo, &hi) ? lo : 0u;
}

// Normalizes the segment whose head is the unit at s (a char that is not active, or a piece start).  False: it holds more than
// NFC_SEG_MAX chars or pieces (or would outgrow three times its source bytes, which no canonical decomposition does; NFK_GROWTH times in
// K mode) -- nothing is valid then.
template <bool K = false>
TK_HD_OUTLINE bool nfc_segment(const NfcTables& t, const uint8_t* text, int64_t n, const nfc_mask_t* bound, int64_t s, NfcSeg& g) {
    int np = 0, nsrc = 0;
    int64_t p = s;
    while (p < n) {
        if (nsrc && nfc_bit(bound, p)) break;
        uint32_t l;
        const uint32_t cp = nfc_decode(text, n, p, &l);
        const uint32_t f = nfc_flags(t, cp);
        if (nsrc && nfc_head<K>(t, cp, f)) break;
        if constexpr (K) {                                      // (the full compatibility decomposition, of any length up to NFKC_MAX_DECOMP)
            if (nsrc == NFC_SEG_MAX) return false;
            uint32_t hd[3] = {cp, 0u, 0u}, off = 0u, cnt = 1u;
            const uint32_t* dp = hd;
            if (f & NFC_F_DECOMP) {
                if (cp - NFC_S_BASE < NFC_S_N) {
                    const uint32_t x = cp - NFC_S_BASE;
                    hd[0] = NFC_L_BASE + x / (NFC_V_N * NFC_T_N);
                    hd[1] = NFC_V_BASE + (x % (NFC_V_N * NFC_T_N)) / NFC_T_N;
                    hd[2] = NFC_T_BASE + x % NFC_T_N;
                    cnt = (x % NFC_T_N) ? 3u : 2u;
                } else if (nfk_map(t, cp, &off, &cnt)) dp = t.kflat + off;
                else cnt = 1u;
            }
            for (uint32_t q = 0; q < cnt; ++q) {
                if (np == NFC_SEG_MAX) return false;
                g.cp[np] = dp[q];
                g.rank[np] = (uint8_t)(((f & NFC_F_DECOMP) ? nfc_flags(t, dp[q]) : f) & NFC_F_RANK);
                g.chg[np] = (int8_t)(q ? 1 : 0);
                ++np;
            }
            g.src[nsrc++] = (uint8_t)(p - s);
            p += l;
            continue;
        }
        // (Lowercase in front of NFD: what it makes of the char are the source chars NFD sees, each aligned to the char)
        uint32_t lc[3] = {cp, 0u, 0u};
        const int nl = (t.mode & NFD_LOWER_FIRST) ? nfd_lower(t, cp, lc) : 1;
        for (int u = 0; u < nl; ++u) {
            if (nsrc == NFC_SEG_MAX) return false;
            const uint32_t c = lc[u], fc = c == cp ? f : nfc_flags(t, c);
            uint32_t d[4] = {c, NFC_FILL, NFC_FILL, NFC_FILL};
            if (fc & NFC_F_DECOMP) {
                if (c - NFC_S_BASE < NFC_S_N) {
                    const uint32_t x = c - NFC_S_BASE;
                    d[0] = NFC_L_BASE + x / (NFC_V_N * NFC_T_N);
                    d[1] = NFC_V_BASE + (x % (NFC_V_N * NFC_T_N)) / NFC_T_N;
                    if (x % NFC_T_N) d[2] = NFC_T_BASE + x % NFC_T_N;
                } else {
                    uint32_t lo, hi;
                    if (nfc_map(t, c, 0u, &lo, &hi)) {
                        const unsigned long long v = ((unsigned long long)hi << 32) | lo;
                        d[0] = (uint32_t)(v & NFC_FILL); d[1] = (uint32_t)((v >> 21) & NFC_FILL); d[2] = (uint32_t)((v >> 42) & NFC_FILL);
                        if (d[2] != NFC_FILL && nfc_map(t, c, 1u, &lo, &hi)) d[3] = lo;
                    }
                }
            }
            for (int q = 0; q < 4 && d[q] != NFC_FILL; ++q) {
                if (np == NFC_SEG_MAX) return false;
                g.cp[np] = d[q];
                g.rank[np] = (uint8_t)(((fc & NFC_F_DECOMP) ? nfc_flags(t, d[q]) : fc) & NFC_F_RANK);
                g.chg[np] = (int8_t)(q ? 1 : 0);
                ++np;
            }
            g.src[nsrc++] = (uint8_t)(p - s);
        }
        p += l;
    }
    g.e = p;
    // canonical ordering: a stable sort by class of every run of non-starters (a starter never moves, nothing moves across one)
    for (int k = 1; k < np; ++k) {
        const uint8_t r = g.rank[k];
        if (!r) continue;
        const uint32_t c = g.cp[k];
        const int8_t h = g.chg[k];
        int j = k - 1;
        while (j >= 0 && g.rank[j] > r) { g.cp[j + 1] = g.cp[j]; g.rank[j + 1] = g.rank[j]; g.chg[j + 1] = g.chg[j]; --j; }
        g.cp[j + 1] = c; g.rank[j + 1] = r; g.chg[j + 1] = h;
    }
    // composition, in place: out[0, no) is final, the composee is held aside, the chars it could not take wait at out[no + 1, no + 1 + nb)
    int no = 0, nb = 0;
    bool have = false;
    uint32_t kc = 0, last = 0;                             // last: class of the char buffered last (0: none is buffered)
    int kh = 0;
    const bool nfd = (t.mode & NFD_MODE) != 0u;
    if (nfd) {                                             // NFD: the ordered pieces are the output; Lowercase behind it maps each to one char
        no = np;
        if (t.mode & NFD_LOWER_LAST)
            for (int k = 0; k < np; ++k) {
                uint32_t lc[3];
                if (nfd_lower(t, g.cp[k], lc) != 1) return false;
                g.cp[k] = lc[0];
            }
    }
    for (int i = 0; i < np && !nfd; ++i) {
        const uint32_t c = g.cp[i], r = g.rank[i];
        const int h = g.chg[i];
        if (!have) {
            if (r) { g.cp[no] = c; g.chg[no] = (int8_t)h; ++no; continue; }
            have = true; kc = c; kh = h;
            continue;
        }
        const bool blocked = nb > 0 && last >= r;
        const uint32_t m = blocked ? 0u : nfc_compose(t, kc, c);
        if (m) { kc = m; kh = kh + h - 1; continue; }
        if (r == 0u) {                                       // a starter the composee does not take: the composee and what waits go out
            g.cp[no] = kc; g.chg[no] = (int8_t)kh;
            no += 1 + nb; nb = 0; last = 0u;
            kc = c; kh = h;
            continue;
        }
        g.cp[no + 1 + nb] = c; g.chg[no + 1 + nb] = (int8_t)h; ++nb;
        last = r;
    }
    if (have) { g.cp[no] = kc; g.chg[no] = (int8_t)kh; no += 1 + nb; }
    // alignment by position in the stream of source chars
    int ptr = 0;
    uint32_t ob = 0;
    for (int k = 0; k < no; ++k) {
        const int h = g.chg[k];
        if (h > 0) g.al[k] = g.src[ptr > 0 ? ptr - 1 : 0];
        else {
            g.al[k] = g.src[ptr < nsrc ? ptr : nsrc - 1];
            ptr += 1 - h;
        }
        ob += nfc_utf8_len(g.cp[k]);
    }
    if (t.mode & NFC_LOWER) {                              // to_lowercase of every composed char, back to front in place
        uint32_t lc[3];
        int add = 0;
        for (int k = 0; k < no; ++k) add += nfd_lower(t, g.cp[k], lc) - 1;
        if (no + add > NFC_SEG_MAX) return false;
        ob = 0;
        for (int k = no - 1, w = no + add; k >= 0; --k) {
            const int nl = nfd_lower(t, g.cp[k], lc);
            const uint8_t al = g.al[k];
            w -= nl;
            for (int u = 0; u < nl; ++u) { g.cp[w + u] = lc[u]; g.al[w + u] = al; ob += nfc_utf8_len(lc[u]); }
        }
        no += add;
    }
    g.n = no;
    g.obytes = ob;
    return ob <= (K ? NFK_GROWTH : 3u) * (uint32_t)(g.e - s);
}

}  // namespace tkamd
