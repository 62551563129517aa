// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after nfc.hip and precompiled.hip;
// it is not compiled on its own).  The NFKC normalizer in front of the "▁" front: the K mode of the NFC core.

// =================================================================================================
// NFKC (normalizers/unicode.rs -> unicode-normalization-alignments), nfc_core.hpp for the rules and the widened head rule.
// The same two passes as k_nfc_count / k_nfc_write over the K = true lane routines, with the 16-bit lane totals of PcOlen (a lane of 16 source bytes may
// stand for 16 x NFK_GROWTH = 176 output bytes; the byte per source byte still holds its NFK_GROWTH).  k_pc_check_len stands between
// the scan and the write, as behind Precompiled.
// =================================================================================================
__global__ __launch_bounds__(256) void k_nfkc_count(NfcArgs a, uint8_t* __restrict__ olen, uint16_t* __restrict__ ltot, uint32_t* __restrict__ wsum, int* __restrict__ err) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * NFC_LANE;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    bool plain = false;
    if (i0 < a.n_bytes) {
        const Unaligned16 t = *(const Unaligned16*)(a.text + i0);
        const uint32_t vb = a.verbatim ? mask16(a.verbatim, i0) : 0u;
        if (vb == 0u && i0 + NFC_LANE <= a.n_bytes) plain = nfc_lane_plain(a, i0, ((t.a | t.b | t.c | t.d) & SW_H) == 0u);
        if (plain) o[0] = o[1] = o[2] = o[3] = SW_1;
        else {
            nfc_count_lane<true>(a, i0, vb, o, err);
            *(uint4*)(olen + i0) = make_uint4(o[0], o[1], o[2], o[3]);        // (the per-byte counts only where the lane is not plain)
        }
    }
    uint32_t sum = 0u;                                                        // (<= 176: the bytes' sums do not fit the multiply trick's byte)
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += (o[k] & 0xFFu) + ((o[k] >> 8) & 0xFFu) + ((o[k] >> 16) & 0xFFu) + (o[k] >> 24);
    if (i0 < a.n_bytes) ltot[i0 >> 4] = (uint16_t)(sum | (plain ? PC_LTOT_PLAIN : 0u));
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    if ((threadIdx.x & 3) == 0 && i0 <= a.n_bytes) wsum[i0 >> 6] = sum;
}

__global__ __launch_bounds__(256) void k_nfkc_write(NfcArgs a, PcOlen olen, const uint32_t* __restrict__ wbase, const int64_t* __restrict__ x_len, const int* __restrict__ err,
                                                    uint8_t* __restrict__ ntext, uint32_t* __restrict__ nos) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * NFC_LANE;
    const uint32_t len = (uint32_t)*x_len;                   // (0 behind k_pc_check_len's refusal: nobody writes)
    const uint32_t lt = (i0 < a.n_bytes && len != 0u) ? (uint32_t)olen.ltot[i0 >> 4] : 0u;
    const uint32_t tot = lt & 0x7FFFu;
    const int lane = lane_id();
    const uint32_t t1 = (uint32_t)__shfl_up((int)tot, 1, 64), t2 = (uint32_t)__shfl_up((int)tot, 2, 64), t3 = (uint32_t)__shfl_up((int)tot, 3, 64);
    const int sub = lane & 3;
    if (!tot) return;
    const uint32_t pos = wbase[i0 >> 6] + (sub >= 1 ? t1 : 0u) + (sub >= 2 ? t2 : 0u) + (sub >= 3 ? t3 : 0u);
    if (pos + tot > len) return;                             // (cannot be: the scan's total is the sum of the lanes')
    if (lt & PC_LTOT_PLAIN) {
        const Unaligned16 t = *(const Unaligned16*)(a.text + i0);
        *(Unaligned16*)(ntext + pos) = t;
        if (nos) {
            const uint32_t b0 = (uint32_t)i0;
            if (((t.a | t.b | t.c | t.d) & SW_H) == 0u) {
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
    nfc_write_lane<true>(a, i0, a.verbatim ? mask16(a.verbatim, i0) : 0u, o, pos, (*err & ERR_NFC_SEGMENT) != 0, ntext, nos);
}
