// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers and bert_norm.hip; it is not compiled on its own).  The NFC normalizer in front of byte-level BPE.

// =================================================================================================
// NFC (normalizers/unicode.rs -> tokenizer/normalizer.rs:461-464), nfc_core.hpp for the rules.
// Almost all text IS NFC, so a batch is first run with X = the text as it came and ONE read of it: k_nfc_check, the exact quick
// check, leaves NOTE_NFC_SEEN when some lane cannot vouch for its bytes, and the host then runs the batch again through the general
// path below (run_pipeline's speculation, like the added tokens').
// The general path has the BertNormalizer's shape -- k_nfc_count sizes the output (BnOlen: a byte per source byte where a lane is
// not plain, a total per 16-byte lane, a sum per 64-byte word), the scan places the words, k_nfc_write emits the text with the source
// char of every byte -- so k_bn_doc_offsets, k_zero_tail and the match translation serve unchanged.  A segment (nfc_core.hpp) is
// normalized by the lane that holds its first byte; its output bytes are charged to its own source bytes (nfc_charge: at most three a
// byte, so a lane's total stays within the 7 bits of ltot), which every lane holding a byte of it works out for itself from the same
// rules -- no lane waits for another.  The segment routine with its 48-entry arrays sits behind calls that are not inlined: lanes of
// plain text never reach them.
// K mode (NFKC in front of the "▁" front, nfc_core.hpp): kernels of its own, k_nfkc_count / k_nfkc_write (kernels/nfkc.hip), over the K = true instantiations
// of the same lane routines -- no branch on it inside the NFC / NFD kernels.  A source byte may stand for NFK_GROWTH output bytes there,
// so a lane's total is 16 bits wide: the Precompiled normalizer's layout (PcOlen, kernels/precompiled.hip), whose length backstop,
// document CSR and match translation serve unchanged.
// =================================================================================================
struct NfcArgs {
    NfcTables nt;
    const uint8_t* text;
    int64_t n_bytes;
    const unsigned long long* verbatim;      // bytes of the raw pass's added-token matches (copied as they are), or null
    const unsigned long long* bound;         // piece starts: document starts, every verbatim byte, the byte behind a verbatim byte
};

// one lane takes 16 bytes; all-ASCII lanes are done with the four loaded words
__global__ __launch_bounds__(256) void k_nfc_check(NfcTables nt, const uint8_t* __restrict__ text, int64_t n_bytes, int* __restrict__ note) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * NFC_LANE;
    bool bad = false;
    if (i0 < n_bytes) {
        const Unaligned16 t = *(const Unaligned16*)(text + i0);                 // (any alignment; readable TEXT_PAD bytes past the end)
        bool look = ((t.a | t.b | t.c | t.d) & SW_H) != 0u;
        if (nt.mode & NFC_LOWER) {                            // (Lowercase behind NFC: an upper-case ASCII letter changes too)
            const uint32_t x[4] = {t.a, t.b, t.c, t.d};
#pragma unroll
            for (int k = 0; k < 4; ++k) look = look || (~sw_lt(x[k], 0x41u) & sw_lt(x[k], 0x5Bu) & SW_H) != 0u;
        }
        if (look) bad = nfc_check_lane(nt, text, n_bytes, i0);
    }
    if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(note, NOTE_NFC_SEEN);
}

// bound[w] = document starts | verbatim | verbatim << 1, in place over the document-start mask
__global__ void k_nfc_bound(unsigned long long* __restrict__ dmask, const unsigned long long* __restrict__ verbatim, int64_t n_words) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words || !verbatim) return;
    const unsigned long long v = verbatim[w], up = w > 0 ? verbatim[w - 1] >> 63 : 0ull;
    dmask[w] |= v | (v << 1) | up;
}

// Is the lane sixteen bytes of units none of which is active, with no active unit right behind it, none verbatim?  Then every byte is
// one output byte: the lane is copied.
__device__ __forceinline__ bool nfc_lane_plain(const NfcArgs& a, int64_t i0, bool ascii) {
    const int64_t i1 = i0 + NFC_LANE;
    int64_t p = i1;
    if (!ascii) {
        p = nfc_unit_start(a.text, a.n_bytes, i0);
        while (p < i1) {
            uint32_t l;
            const uint32_t cp = nfc_decode(a.text, a.n_bytes, p, &l), f = nfc_flags(a.nt, cp);
            if (f & NFC_F_ACTIVE) return false;
            if (a.nt.mode && nfd_changes(a.nt, cp, f)) return false;      // (NFD mode: an upper-case ASCII letter among them too -- only all-ASCII lanes are lowercased on the copy)
            p += l;
        }
    }
    if (p >= a.n_bytes || a.text[p] < 0x80u || nfc_bit(a.bound, p)) return true;
    uint32_t l;
    return !(nfc_flags(a.nt, nfc_decode(a.text, a.n_bytes, p, &l)) & NFC_F_ACTIVE);
}

// the segment that holds the unit starting at cs: [*s, *e) and its output bytes; a refused one (ERR_NFC_SEGMENT) is the unit itself, unchanged
template <bool K = false>
__device__ __forceinline__ void nfc_segment_of(const NfcArgs& a, int64_t cs, NfcSeg& g, int64_t* s, int64_t* e, uint32_t* O, int* __restrict__ err) {
    uint32_t l;
    const int64_t h = nfc_seg_start<K>(a.nt, a.text, a.n_bytes, a.bound, cs);
    if (h >= 0) {
        const uint32_t f = nfc_flags(a.nt, nfc_decode(a.text, a.n_bytes, h, &l));
        if (nfc_trivial<K>(a.nt, a.text, a.n_bytes, a.bound, h, f, l)) { *s = h; *e = h + l; *O = l; return; }
        if (nfc_segment<K>(a.nt, a.text, a.n_bytes, a.bound, h, g)) { *s = h; *e = g.e; *O = g.obytes; return; }
    }
    if (err) atomicOr(err, ERR_NFC_SEGMENT);
    nfc_decode(a.text, a.n_bytes, cs, &l);
    *s = cs; *e = cs + l; *O = l;
}

// output bytes of each of the lane's bytes, the general way
template <bool K = false>
__device__ __noinline__ void nfc_count_lane(const NfcArgs& a, int64_t i0, uint32_t vb, uint32_t* __restrict__ o, int* __restrict__ err) {
    NfcSeg g;
    int64_t s = 0, e = -1;
    uint32_t O = 0;
    const int nv = (int)min((int64_t)NFC_LANE, a.n_bytes - i0);
    for (int j = 0; j < nv; ++j) {
        const int64_t i = i0 + j;
        uint32_t c = 1u;
        if (!((vb >> j) & 1u)) {
            if (i >= e) nfc_segment_of<K>(a, nfc_unit_start(a.text, a.n_bytes, i), g, &s, &e, &O, err);
            c = K ? nfc_charge_g<NFK_GROWTH>((uint32_t)(i - s), O, (uint32_t)(e - s)) : nfc_charge((uint32_t)(i - s), O, (uint32_t)(e - s));
        }
        o[j >> 2] |= c << (8 * (j & 3));
    }
}

__global__ __launch_bounds__(256) void k_nfc_count(NfcArgs a, uint8_t* __restrict__ olen, uint8_t* __restrict__ ltot, uint32_t* __restrict__ wsum, int* __restrict__ err) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * NFC_LANE;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    bool plain = false;
    if (i0 < a.n_bytes) {
        const Unaligned16 t = *(const Unaligned16*)(a.text + i0);
        const uint32_t vb = a.verbatim ? mask16(a.verbatim, i0) : 0u;
        if (vb == 0u && i0 + NFC_LANE <= a.n_bytes) plain = nfc_lane_plain(a, i0, ((t.a | t.b | t.c | t.d) & SW_H) == 0u);
        if (plain) o[0] = o[1] = o[2] = o[3] = SW_1;
        else {
            nfc_count_lane(a, i0, vb, o, err);
            *(uint4*)(olen + i0) = make_uint4(o[0], o[1], o[2], o[3]);        // (the per-byte counts only where the lane is not plain: BnOlen)
        }
    }
    uint32_t sum = ((o[0] * SW_1) >> 24) + ((o[1] * SW_1) >> 24) + ((o[2] * SW_1) >> 24) + ((o[3] * SW_1) >> 24);      // (<= 48: three a byte)
    if (i0 < a.n_bytes) ltot[i0 >> 4] = (uint8_t)(sum | (plain ? BN_LTOT_PLAIN : 0u));
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    if ((threadIdx.x & 3) == 0 && i0 <= a.n_bytes) wsum[i0 >> 6] = sum;
}

__device__ __forceinline__ void nfc_copy_unit(const uint8_t* __restrict__ text, int64_t i, uint32_t l, uint32_t pos, uint8_t* __restrict__ ntext, uint32_t* __restrict__ nos) {
    for (uint32_t z = 0; z < l; ++z) { ntext[pos + z] = text[i + z]; if (nos) nos[pos + z] = (uint32_t)i; }
}

// writes what the lane's bytes stand for, the general way: a verbatim byte itself; the head of a segment the whole segment, at the
// place its first byte has; every other unit nothing -- unless its segment was refused (refusals: the error bit is up), then itself
template <bool K = false>
__device__ __noinline__ void nfc_write_lane(const NfcArgs& a, int64_t i0, uint32_t vb, const uint32_t* __restrict__ o, uint32_t pos, bool refusals,
                                            uint8_t* __restrict__ ntext, uint32_t* __restrict__ nos) {
    NfcSeg g;
    const int nv = (int)min((int64_t)NFC_LANE, a.n_bytes - i0);
    for (int j = 0; j < nv; ++j) {
        const int64_t i = i0 + j;
        const uint32_t ob = (o[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        if ((vb >> j) & 1u) {
            ntext[pos] = a.text[i];
            if (nos) nos[pos] = (uint32_t)i;
        } else if (nfc_unit_start(a.text, a.n_bytes, i) == i) {
            uint32_t l;
            const uint32_t f = nfc_flags(a.nt, nfc_decode(a.text, a.n_bytes, i, &l));
            bool head = !(f & NFC_F_ACTIVE);
            if constexpr (K) head = nfc_head<true>(a.nt, nfc_decode(a.text, a.n_bytes, i, &l), f);
            if (i == 0 || nfc_bit(a.bound, i) || head) {
                if (nfc_trivial<K>(a.nt, a.text, a.n_bytes, a.bound, i, f, l) || !nfc_segment<K>(a.nt, a.text, a.n_bytes, a.bound, i, g)) nfc_copy_unit(a.text, i, l, pos, ntext, nos);
                else {
                    uint32_t k = pos;
                    for (int q = 0; q < g.n; ++q) {
                        const uint32_t bl = nfc_utf8_put(ntext + k, g.cp[q]);
                        if (nos) for (uint32_t z = 0; z < bl; ++z) nos[k + z] = (uint32_t)i + g.al[q];
                        k += bl;
                    }
                }
            } else if (refusals) {
                int64_t s, e;
                uint32_t O;
                nfc_segment_of<K>(a, i, g, &s, &e, &O, nullptr);
                if (s == i && e == i + (int64_t)l && ob != 0u) nfc_copy_unit(a.text, i, l, pos, ntext, nos);      // (refused: the unit alone)
            }
        } else if (ob != 0u) {
            // a byte of a unit that began in the lane in front: if that lane was copied whole it wrote its own sixteen bytes only, so
            // the rest of a unit that is a segment of its own (one output byte a source byte) is written here, byte for byte
            const int64_t cs = nfc_unit_start(a.text, a.n_bytes, i);
            if (cs < i0) {
                uint32_t l;
                const uint32_t f = nfc_flags(a.nt, nfc_decode(a.text, a.n_bytes, cs, &l));
                if (nfc_trivial<K>(a.nt, a.text, a.n_bytes, a.bound, cs, f, l)) {
                    ntext[pos] = a.text[i];
                    if (nos) nos[pos] = (uint32_t)cs;
                }
            }
        }
        pos += ob;
    }
}

__global__ __launch_bounds__(256) void k_nfc_write(NfcArgs a, BnOlen olen, const uint32_t* __restrict__ wbase, const int* __restrict__ err,
                                                   uint8_t* __restrict__ ntext, uint32_t* __restrict__ nos) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * NFC_LANE;
    const uint32_t lt = i0 < a.n_bytes ? (uint32_t)olen.ltot[i0 >> 4] : 0u;
    const uint32_t tot = lt & 0x7Fu;
    const int lane = lane_id();
    const uint32_t t1 = (uint32_t)__shfl_up((int)tot, 1, 64), t2 = (uint32_t)__shfl_up((int)tot, 2, 64), t3 = (uint32_t)__shfl_up((int)tot, 3, 64);
    const int sub = lane & 3;
    if (!tot) return;
    const uint32_t pos = wbase[i0 >> 6] + (sub >= 1 ? t1 : 0u) + (sub >= 2 ? t2 : 0u) + (sub >= 3 ? t3 : 0u);
    if (lt & BN_LTOT_PLAIN) {
        const Unaligned16 t = *(const Unaligned16*)(a.text + i0);
        const bool ascii = ((t.a | t.b | t.c | t.d) & SW_H) == 0u;
        if (ascii && (a.nt.mode & NFC_ANY_LOWER)) {                // (Lowercase is a member: A-Z -> a-z on the copy, as in k_bn_write)
            uint32_t x[4] = {t.a, t.b, t.c, t.d};
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] += (~sw_lt(x[k], 0x41u) & sw_lt(x[k], 0x5Bu) & SW_H) >> 2;
            *(Unaligned16*)(ntext + pos) = Unaligned16{x[0], x[1], x[2], x[3]};
        } else *(Unaligned16*)(ntext + pos) = t;
        if (nos) {
            const uint32_t b0 = (uint32_t)i0;
            if (ascii) {
#pragma unroll
                for (int j = 0; j < NFC_LANE; j += 4) *(Unaligned16*)(nos + pos + j) = Unaligned16{b0 + j, b0 + j + 1u, b0 + j + 2u, b0 + j + 3u};
            } else {
                for (int j = 0; j < NFC_LANE; ++j) nos[pos + j] = (uint32_t)nfc_unit_start(a.text, a.n_bytes, i0 + j);      // (every byte of a char: the char's first byte)
            }
        }
        return;
    }
    const uint4 ol = *(const uint4*)(olen.olen + i0);
    const uint32_t o[4] = {ol.x, ol.y, ol.z, ol.w};
    nfc_write_lane(a, i0, a.verbatim ? mask16(a.verbatim, i0) : 0u, o, pos, (*err & ERR_NFC_SEGMENT) != 0, ntext, nos);
}
