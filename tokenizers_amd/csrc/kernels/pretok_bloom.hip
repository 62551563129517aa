// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after kernels/pretok_gpt2.hip, whose
// constants it shares; it is not compiled on its own).  Split(BLOOM's pattern, Isolated) + ByteLevel(use_regex=false) of BLOOM / BLOOMZ
// (PT_BLOOM): one bit-parallel lane kernel.  The rule is purely local -- no undecided bytes, no sequential tier.

// =================================================================================================
// K_pretok_bloom: the pieces BLOOM's Split leaves (pretok_bloom_core.hpp), one lane per 64-bit word of the start mask, in the form of
// k_pretok_gpt2_seq and k_pretok_digits: a lane loads and classifies its own 64 bytes once through a flag LUT in LDS (this kind's own:
// one 32-bit word a byte value), resolves its multi-byte chars, exchanges a few bits with the lanes of the words on either side --
// __shfl_up / __shfl_down inside a wavefront, eight words of LDS and ONE barrier between the wavefronts, and lanes 0 and 1 read the
// bytes beyond the two ends of the workgroup themselves -- and evaluates the rule as mask algebra.  What travels: one 32-bit `up` word
// (5 bits used), one 32-bit `down` word (2 bits used).
// LEAD: the lead-byte mask of the same text rides along, as in k_pretok_gpt2_seq.
// =================================================================================================
template <bool LEAD>
__global__ __launch_bounds__(256) void k_pretok_bloom(const uint8_t* __restrict__ text, int64_t n_bytes_host, const int64_t* __restrict__ len_dev,
                                                      const unsigned long long* __restrict__ docmask, const uint16_t* __restrict__ uc1,
                                                      const uint8_t* __restrict__ uc2, unsigned long long* __restrict__ startmask,
                                                      unsigned long long* __restrict__ leadmask) {
    __shared__ uint32_t lut[256];
    __shared__ uint32_t sh_up[4];                // [v]: what the last lane of wavefront v - 1 hands up ([0]: the word in front of the workgroup)
    __shared__ uint32_t sh_down[4];              // [v]: what the first lane of wavefront v + 1 hands down ([3]: the word behind the workgroup)
    lut[threadIdx.x] = bloom_byte_flags(threadIdx.x);        // 256 threads: one table entry each
    __syncthreads();
    const int64_t n_bytes = len_dev ? *len_dev : n_bytes_host;
    const int64_t n_words_host = (n_bytes_host >> 6) + 1;
    const int64_t w = (int64_t)blockIdx.x * G2_WORDS_PER_BLOCK + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    // the word's own 64 bytes (a word past the text: all zero, no load)
    BloomWord m;
    bloom_word_classify(text, n_bytes, (const uint64_t*)docmask, lut, w, uc1, uc2, m);
    const uint32_t up = bloom_pack_up(m), down = bloom_pack_down(m);
    uint32_t from_below = __shfl_up(up, 1, 64), from_above = __shfl_down(down, 1, 64);
    if (lane == 63 && wave < 3) sh_up[wave + 1] = up;
    if (lane == 0 && wave > 0) sh_down[wave - 1] = down;
    if (threadIdx.x < 2) {
        // the ends of the workgroup: thread 0 the bytes in front of its own word, thread 1 the first byte behind the workgroup's last word
        const int64_t pos = threadIdx.x == 0 ? w << 6 : (w + G2_WORDS_PER_BLOCK - 1) << 6;
        if (threadIdx.x == 0) sh_up[0] = (w > 0 && pos < n_bytes) ? bloom_edge_up(text, pos, lut, uc1, uc2) : 0u;
        else sh_down[3] = pos < n_bytes ? bloom_edge_down(text, pos, (const uint64_t*)docmask, lut, uc1, uc2) : 0u;
    }
    __syncthreads();
    if (lane == 0) from_below = sh_up[wave];
    if (lane == 63) from_above = sh_down[wave];
    uint64_t ld = 0;
    const unsigned long long out = bloom_word_starts(m, from_below, from_above, w, n_bytes, LEAD ? &ld : nullptr);
    if (w < n_words_host) {
        startmask[w] = out;
        if constexpr (LEAD) leadmask[w] = (unsigned long long)ld;
    }
}
