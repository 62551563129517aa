// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after kernels/pretok_gpt2.hip, whose
// constants it shares; it is not compiled on its own).  Split(the CLIP pattern, Removed, inverted) + ByteLevel (PT_CLIP): one bit-parallel
// lane kernel.  The rule is purely local -- no undecided bytes, no sequential tier.

// =================================================================================================
// K_pretok_clip: the CLIP pattern's matches (pretok_clip_core.hpp), one lane per 64-bit word of the start mask and of the END mask, in
// the form of k_pretok_gpt2_seq and k_pretok_digits: a lane loads and classifies its own 64 bytes once through the flag LUT in LDS,
// resolves its multi-byte code points, exchanges 8 bits of every mask with the lanes of the words on either side -- __shfl_up /
// __shfl_down inside a wavefront, a few words of LDS and ONE barrier between the wavefronts, and lanes 0 and 1 classify the 8 bytes
// beyond the two ends of the workgroup themselves -- and evaluates the regex as mask algebra.  What travels is k_pretok_gpt2_seq's: one
// 64-bit `up` word, one 32-bit `down` word.  The word that holds the position n_bytes may have no byte of its own and still gets the end
// bit of the text's last pre-token: its lane takes the left halo like any other.
// LEAD: the lead-byte mask of the same text rides along, as in k_pretok_gpt2_seq.
// =================================================================================================
template <bool LEAD>
__global__ __launch_bounds__(256) void k_pretok_clip(const uint8_t* __restrict__ text, int64_t n_bytes_host, const int64_t* __restrict__ len_dev,
                                                     const unsigned long long* __restrict__ docmask, const uint16_t* __restrict__ uc1,
                                                     const uint8_t* __restrict__ uc2, unsigned long long* __restrict__ startmask,
                                                     unsigned long long* __restrict__ endmask, unsigned long long* __restrict__ leadmask) {
    __shared__ Gpt2Flags lut[256];
    __shared__ unsigned long long sh_up[4];      // [v]: what the last lane of wavefront v - 1 hands up ([0]: the word in front of the workgroup)
    __shared__ uint32_t sh_down[4];              // [v]: what the first lane of wavefront v + 1 hands down ([3]: the word behind the workgroup)
    lut[threadIdx.x] = gpt2_byte_flags(threadIdx.x);         // 256 threads: one table entry each
    __syncthreads();
    const int64_t n_bytes = len_dev ? *len_dev : n_bytes_host;
    const int64_t n_words_host = (n_bytes_host >> 6) + 1;
    const int64_t w = (int64_t)blockIdx.x * G2_WORDS_PER_BLOCK + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    // the word's own 64 bytes (a word past the text: all zero, no load)
    Gpt2Window m;
    const Gpt2Spill spill = gpt2_word_classify(text, n_bytes, (const uint64_t*)docmask, lut, w, uc1, uc2, m);
    const unsigned long long up = gpt2_pack_up(m, spill);
    const uint32_t down = gpt2_pack_down(m);
    unsigned long long from_below = __shfl_up(up, 1, 64);
    uint32_t from_above = __shfl_down(down, 1, 64);
    if (lane == 63 && wave < 3) sh_up[wave + 1] = up;
    if (lane == 0 && wave > 0) sh_down[wave - 1] = down;
    if (threadIdx.x < 2) {
        // the ends of the workgroup: thread 0 the 8 bytes in front of its own word (also when that word is the position n_bytes alone),
        // thread 1 the 8 bytes behind the workgroup's last word
        const int64_t pos = threadIdx.x == 0 ? (w << 6) - 8 : (w + G2_WORDS_PER_BLOCK - 1) << 6;
        const bool there = threadIdx.x == 0 ? (w > 0 && (w << 6) <= n_bytes) : pos < n_bytes;
        Gpt2Halo h{0, 0, 0, 0, 0, 0, 0, 0};
        Gpt2Spill hs{0, 0, 0};
        if (there) h = gpt2_halo_classify(text, n_bytes, (const uint64_t*)docmask, lut, pos, uc1, uc2, &hs);
        if (threadIdx.x == 0) sh_up[0] = gpt2_pack_up(h.L, h.N, h.S, h.SP, h.AP, h.D, hs);
        else sh_down[3] = gpt2_pack_down(h.L, h.S, h.C, h.D);
    }
    __syncthreads();
    if (lane == 0) from_below = sh_up[wave];
    if (lane == 63) from_above = sh_down[wave];
    const Gpt2Halo hl = gpt2_take_left(from_below, w, m);
    const Gpt2Halo hr = gpt2_take_right(from_above, w, n_bytes, spill);
    uint64_t st = 0, en = 0, ld = 0;
    clip_word_masks(m, hl, hr, text, w, n_bytes, &st, &en, LEAD ? &ld : nullptr);
    if (w < n_words_host) {
        startmask[w] = (unsigned long long)st;
        endmask[w] = (unsigned long long)en;
        if constexpr (LEAD) leadmask[w] = (unsigned long long)ld;
    }
}
