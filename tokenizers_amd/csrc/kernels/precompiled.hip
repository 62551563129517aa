// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers, bert_norm.hip and nfc.hip; it is not compiled on its own).  The Precompiled normalizer in front of Unigram.

// =================================================================================================
// Precompiled (normalizers/precompiled.rs), precompiled_core.hpp for the rules.
// The BertNormalizer's shape: k_pc_count sizes the output of every source byte (16 bytes a lane), the scan places the 64-byte words,
// k_pc_write emits the normalized text with the source char of every byte.  What a char becomes is a function of the char and of its
// grapheme cluster (pc_char_out): the lane that holds a char's first byte works it out and charges the output to that byte -- a
// cluster of fewer than 6 bytes that hits the trie whole is charged to its first char, its other chars to nothing -- so no lane waits
// for another and nobody keeps a cluster in arrays.  A lane is PLAIN and is copied with its four loaded words when it is sixteen ASCII
// bytes none of which starts a key, behind an ASCII byte that is no CR in front of an LF: every byte then opens a cluster of its own
// that the trie cannot hit.  Nobody walks the trie for such text.
// A replacement may be long (U+FDFA: 3 bytes -> 33), so the per-lane totals are 16 bits here (PcOlen) where the BertNormalizer's are 7:
// the document CSR and the match translation have forms of their own below; k_zero_tail and the scan serve unchanged.
// k_pc_check_len stands between the scan and the write: a text beyond the host's bound fails the batch and is not written.
// k_pc_lost_fix runs only behind NOTE_PC_LOST: a piece whose first chars became nothing (precompiled_core.hpp) has its entries moved.
// =================================================================================================
struct PcArgs {
    PcTables pt;
    const uint8_t* text;
    int64_t n_bytes;
    const unsigned long long* verbatim;      // bytes of the raw pass's added-token matches (copied as they are), or null
    const unsigned long long* bound;         // piece starts: document starts, every verbatim byte, the byte behind a verbatim byte
};
constexpr uint32_t PC_LTOT_PLAIN = 0x8000u;
struct PcOlen { const uint8_t* olen; const uint16_t* ltot; };
__device__ __forceinline__ uint32_t pc_olen_before(const PcOlen& o, int64_t g) {
    uint32_t r = 0;
    const int64_t w0 = g & ~(int64_t)63, l0 = g & ~(int64_t)15;
    for (int64_t q = w0; q < l0; q += 16) r += o.ltot[q >> 4] & 0x7FFFu;
    if (o.ltot[l0 >> 4] & PC_LTOT_PLAIN) r += (uint32_t)(g - l0);
    else for (int64_t q = l0; q < g; ++q) r += o.olen[q];
    return r;
}
// (never beyond the text's length: behind k_pc_check_len that is 0 for a text that would not fit its buffer)
__device__ __forceinline__ uint32_t pc_position(const PcOlen& o, const uint32_t* __restrict__ wbase, int64_t n_bytes, const int64_t* __restrict__ x_len, int64_t g) {
    const uint32_t len = (uint32_t)*x_len;
    if (g >= n_bytes) return len;
    return min(wbase[g >> 6] + pc_olen_before(o, g), len);
}

// The backstop behind the scan, in front of every write: the host sized the normalized text's buffers by the growth the loader found
// in the charsmap (HostModel::pc_growth).  Should the text the count pass sized not fit them all the same, the batch fails with
// ERR_INTERNAL, the text's length becomes 0 and k_pc_write writes nothing -- a wrong bound never turns into a store outside a buffer.
__global__ void k_pc_check_len(int64_t* __restrict__ x_len, int64_t cap, int* __restrict__ err) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && (*x_len > cap || *x_len < 0)) {
        atomicOr(err, ERR_INTERNAL);
        *x_len = 0;
    }
}

// output bytes of the source byte i (b = text[i], not verbatim): a char's whole output on its first byte
__device__ __forceinline__ uint32_t pc_count_byte(const PcArgs& a, int64_t i, uint32_t b, int* __restrict__ note) {
    if ((b & 0xC0u) == 0x80u && nfc_unit_start(a.text, a.n_bytes, i) != i) return 0u;
    uint32_t l, ro = 0u, rl = 0u;
    int64_t se;
    const PcOut k = pc_char_out(a.pt, a.text, a.n_bytes, a.bound, i, &ro, &rl, &se);
    if (k == PC_COPY) { nfc_decode(a.text, a.n_bytes, i, &l); return l; }
    if (k == PC_NONE) return 0u;
    if (rl == 0u && pc_piece_start(a.bound, i)) atomicOr(note, NOTE_PC_LOST);
    return rl;
}

__device__ __forceinline__ bool pc_lane_plain(const PcArgs& a, int64_t i0, const uint32_t* __restrict__ x) {
    if (((x[0] | x[1] | x[2] | x[3]) & SW_H) != 0u || i0 + PC_LANE > a.n_bytes) return false;
    if (i0 > 0) {
        const uint32_t pb = a.text[i0 - 1];
        if (pb >= 0x80u || (pb == 13u && (x[0] & 0xFFu) == 10u)) return false;
    }
    bool key = false;
#pragma unroll
    for (int j = 0; j < PC_LANE; ++j) key = key || pc_first(a.pt, (x[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    return !key;
}

__global__ __launch_bounds__(256) void k_pc_count(PcArgs a, uint8_t* __restrict__ olen, uint16_t* __restrict__ ltot, uint32_t* __restrict__ wsum, int* __restrict__ note) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PC_LANE;
    uint32_t sum = 0u;
    bool plain = false;
    if (i0 < a.n_bytes) {
        const Unaligned16 t = *(const Unaligned16*)(a.text + i0);                 // (any alignment; readable TEXT_PAD bytes past the end)
        const uint32_t x[4] = {t.a, t.b, t.c, t.d};
        const uint32_t vb = a.verbatim ? mask16(a.verbatim, i0) : 0u;
        plain = vb == 0u && pc_lane_plain(a, i0, x);
        if (plain) sum = PC_LANE;
        else {
            uint32_t o[4] = {0u, 0u, 0u, 0u};
            const int nv = (int)min((int64_t)PC_LANE, a.n_bytes - i0);
            for (int j = 0; j < nv; ++j) {
                const uint32_t c = ((vb >> j) & 1u) ? 1u : pc_count_byte(a, i0 + j, (x[j >> 2] >> (8 * (j & 3))) & 0xFFu, note);
                o[j >> 2] |= c << (8 * (j & 3));
                sum += c;
            }
            *(uint4*)(olen + i0) = make_uint4(o[0], o[1], o[2], o[3]);           // (the per-byte counts only where the lane is not plain)
        }
        ltot[i0 >> 4] = (uint16_t)(sum | (plain ? PC_LTOT_PLAIN : 0u));            // (<= 16 x PC_REP_MAX)
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    if ((threadIdx.x & 3) == 0 && i0 <= a.n_bytes) wsum[i0 >> 6] = sum;
}

__global__ __launch_bounds__(256) void k_pc_write(PcArgs a, PcOlen olen, const uint32_t* __restrict__ wbase, const int64_t* __restrict__ x_len, uint8_t* __restrict__ ntext,
                                                  uint32_t* __restrict__ nos) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PC_LANE;
    const uint32_t len = (uint32_t)*x_len;                   // (0 behind k_pc_check_len's refusal: nobody writes)
    const uint32_t lt = (i0 < a.n_bytes && len != 0u) ? (uint32_t)olen.ltot[i0 >> 4] : 0u;
    const uint32_t tot = lt & 0x7FFFu;
    const int lane = lane_id();
    const uint32_t t1 = (uint32_t)__shfl_up((int)tot, 1, 64), t2 = (uint32_t)__shfl_up((int)tot, 2, 64), t3 = (uint32_t)__shfl_up((int)tot, 3, 64);
    const int sub = lane & 3;
    if (!tot) return;
    uint32_t pos = wbase[i0 >> 6] + (sub >= 1 ? t1 : 0u) + (sub >= 2 ? t2 : 0u) + (sub >= 3 ? t3 : 0u);
    if (pos + tot > len) return;                             // (cannot be: the scan's total is the sum of the lanes')
    if (lt & PC_LTOT_PLAIN) {
        *(Unaligned16*)(ntext + pos) = *(const Unaligned16*)(a.text + i0);
        if (nos) {
            const uint32_t b0 = (uint32_t)i0;
#pragma unroll
            for (int j = 0; j < PC_LANE; j += 4) *(Unaligned16*)(nos + pos + j) = Unaligned16{b0 + j, b0 + j + 1u, b0 + j + 2u, b0 + j + 3u};
        }
        return;
    }
    const uint4 ol = *(const uint4*)(olen.olen + i0);
    const uint32_t o[4] = {ol.x, ol.y, ol.z, ol.w};
    const uint32_t vb = a.verbatim ? mask16(a.verbatim, i0) : 0u;
    const int nv = (int)min((int64_t)PC_LANE, a.n_bytes - i0);
    for (int j = 0; j < nv; ++j) {
        const uint32_t ob = (o[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        if (!ob) continue;
        const int64_t i = i0 + j;
        if ((vb >> j) & 1u) {
            ntext[pos] = a.text[i];
            if (nos) nos[pos] = (uint32_t)i;
            ++pos;
            continue;
        }
        uint32_t ro = 0u, rl = 0u;
        int64_t se = 0;
        if (pc_char_out(a.pt, a.text, a.n_bytes, a.bound, i, &ro, &rl, &se) == PC_REP) {
            // the replacement's i-th char takes the i-th source char of what it replaces, the chars beyond the last source char that one
            // (an inserted last char in front of chars that become nothing takes the first of those: pc_tail_moves)
            int64_t q = i;
            bool inserted = false;
            for (uint32_t z = 0; z < rl;) {
                uint32_t cl, ql;
                nfc_decode(a.pt.rep + ro, rl, z, &cl);
                const uint32_t src = (uint32_t)((nos && inserted && z + cl == rl && pc_tail_moves(a.pt, a.text, a.n_bytes, a.bound, se)) ? se : q);
                for (uint32_t y = 0; y < cl; ++y) { ntext[pos + z + y] = a.pt.rep[ro + z + y]; if (nos) nos[pos + z + y] = src; }
                z += cl;
                nfc_decode(a.text, a.n_bytes, q, &ql);
                if (q + (int64_t)ql < se) q += ql; else inserted = true;
            }
        } else {
            for (uint32_t y = 0; y < ob; ++y) { ntext[pos + y] = a.text[i + y]; if (nos) nos[pos + y] = (uint32_t)i; }
        }
        pos += ob;
    }
}

// Behind NOTE_PC_LOST, with offsets: a lane per word of the bound mask looks at the pieces that start in it; one whose first chars
// became nothing has every entry of its output moved that many source chars back (one lane walks the piece: such pieces are the
// documents that begin with U+FEFF, few and far between).
__global__ __launch_bounds__(256) void k_pc_lost_fix(PcArgs a, PcOlen olen, const uint32_t* __restrict__ wbase, const int64_t* __restrict__ x_len, const int* __restrict__ note,
                                                     uint32_t* __restrict__ nos) {
    if (!(*note & NOTE_PC_LOST)) return;
    const int64_t n_words = (a.n_bytes + 63) >> 6;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * 256) {
        unsigned long long m = a.bound[w] | (w == 0 ? 1ull : 0ull);
        if (a.verbatim) m &= ~a.verbatim[w];
        for (; m; m &= m - 1ull) {
            const int64_t p = (w << 6) + (__ffsll(m) - 1);
            if (p >= a.n_bytes || !pc_first(a.pt, a.text[p])) continue;
            const uint32_t lost = pc_lost_chars(a.pt, a.text, a.n_bytes, a.bound, p);
            if (!lost) continue;
            int64_t e = p + 1;                                               // the piece's end: the next bound bit, or the text's
            while (e < a.n_bytes && !nfc_bit(a.bound, e)) {
                const unsigned long long rest = a.bound[e >> 6] >> (e & 63);
                e = rest ? e + (__ffsll(rest) - 1) : ((e >> 6) + 1) << 6;
            }
            if (e > a.n_bytes) e = a.n_bytes;
            const uint32_t k1 = pc_position(olen, wbase, a.n_bytes, x_len, e);
            for (uint32_t k = pc_position(olen, wbase, a.n_bytes, x_len, p); k < k1; ++k) nos[k] = (uint32_t)pc_chars_back(a.text, a.n_bytes, nos[k], lost);
        }
    }
}

// document CSR in normalized coordinates (k_bn_doc_offsets over PcOlen)
__global__ void k_pc_doc_offsets(const int64_t* __restrict__ doc_off, int64_t n_docs, int64_t n_bytes, PcOlen olen, const uint32_t* __restrict__ wbase,
                                 const int64_t* __restrict__ x_len, int64_t* __restrict__ ndoc_off) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_docs) return;
    int64_t g = doc_off[d];
    if (g < 0) g = 0;
    ndoc_off[d] = pc_position(olen, wbase, n_bytes, x_len, g);
}
// match list entries from the raw text into the normalized text (k_translate_matches_norm over PcOlen)
__global__ void k_pc_translate_matches(uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list, PcOlen olen, const uint32_t* __restrict__ wbase, int64_t n_bytes,
                                       const int64_t* __restrict__ x_len) {
    const uint32_t n = *n_list;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        list[4 * i] = pc_position(olen, wbase, n_bytes, x_len, list[4 * i]);
        list[4 * i + 1] = pc_position(olen, wbase, n_bytes, x_len, list[4 * i + 1]);
    }
}
