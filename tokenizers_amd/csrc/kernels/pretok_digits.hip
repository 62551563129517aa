// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after kernels/pretok_gpt2.hip, whose
// constants it shares; it is not compiled on its own).  Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family
// (PT_DIGITS_GPT2): one bit-parallel lane kernel.  The rule is purely local -- no undecided bytes, no sequential tier.

// =================================================================================================
// K_pretok_digits: the GPT-2 start predicate inside the pieces the Digits pre-tokenizer cuts, one lane per 64-bit word of the start mask,
// in the form of k_pretok_gpt2_seq: a lane loads and classifies its own 64 bytes once through the flag LUT in LDS, resolves its
// multi-byte code points (here also for char::is_numeric, UC_RUST_N: the mask Nr), exchanges 8 bits of every mask with the lanes of the
// words on either side -- __shfl_up / __shfl_down inside a wavefront, a few words of LDS and ONE barrier between the wavefronts, and
// lanes 0 and 1 classify the 8 bytes beyond the two ends of the workgroup themselves -- and evaluates the regex as mask algebra.  The
// piece edges E join the document mask before that algebra (pretok_digits_core.hpp).  What travels beyond k_pretok_gpt2_seq's words:
// four bits of Nr in free bits of the 64-bit `up` word and one more 32-bit `down` word.
// INDIVIDUAL: Digits(individual_digits=true).  LEAD: the lead-byte mask of the same text rides along, as in k_pretok_gpt2_seq.
// =================================================================================================
template <bool INDIVIDUAL, bool LEAD>
__global__ __launch_bounds__(256) void k_pretok_digits(const uint8_t* __restrict__ text, int64_t n_bytes_host, const int64_t* __restrict__ len_dev,
                                                       const unsigned long long* __restrict__ docmask, const uint16_t* __restrict__ uc1,
                                                       const uint8_t* __restrict__ uc2, unsigned long long* __restrict__ startmask,
                                                       unsigned long long* __restrict__ leadmask) {
    __shared__ Gpt2Flags lut[256];
    __shared__ unsigned long long sh_up[4];      // [v]: what the last lane of wavefront v - 1 hands up ([0]: the word in front of the workgroup)
    __shared__ uint32_t sh_down[4], sh_down_nr[4];   // [v]: what the first lane of wavefront v + 1 hands down ([3]: the word behind the workgroup)
    lut[threadIdx.x] = gpt2_byte_flags(threadIdx.x);         // 256 threads: one table entry each
    __syncthreads();
    const int64_t n_bytes = len_dev ? *len_dev : n_bytes_host;
    const int64_t n_words_host = (n_bytes_host >> 6) + 1;
    const int64_t w = (int64_t)blockIdx.x * G2_WORDS_PER_BLOCK + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    // the word's own 64 bytes (a word past the text: all zero, no load)
    Gpt2Window m;
    uint64_t Nr;
    const DigitsSpill spill = digits_word_classify(text, n_bytes, (const uint64_t*)docmask, lut, w, uc1, uc2, m, &Nr);
    const unsigned long long up = digits_pack_up<INDIVIDUAL>(m, Nr, spill);
    const uint32_t down = gpt2_pack_down(m), down_nr = (uint32_t)Nr & 0xFFu;
    unsigned long long from_below = __shfl_up(up, 1, 64);
    uint32_t from_above = __shfl_down(down, 1, 64), from_above_nr = __shfl_down(down_nr, 1, 64);
    if (lane == 63 && wave < 3) sh_up[wave + 1] = up;
    if (lane == 0 && wave > 0) { sh_down[wave - 1] = down; sh_down_nr[wave - 1] = down_nr; }
    if (threadIdx.x < 2) {
        // the ends of the workgroup: thread 0 the 8 bytes in front of its own word, thread 1 the 8 bytes behind the workgroup's last word
        const int64_t pos = threadIdx.x == 0 ? (w << 6) - 8 : (w + G2_WORDS_PER_BLOCK - 1) << 6;
        const bool there = threadIdx.x == 0 ? (w > 0 && (w << 6) < n_bytes) : pos < n_bytes;
        Gpt2Halo h{0, 0, 0, 0, 0, 0, 0, 0};
        DigitsSpill hs{{0, 0, 0}, 0};
        uint32_t nr8 = 0;
        if (there) h = digits_halo_classify<INDIVIDUAL>(text, n_bytes, (const uint64_t*)docmask, lut, pos, uc1, uc2, &hs, &nr8);
        if (threadIdx.x == 0) sh_up[0] = digits_pack_up(h, hs);
        else { sh_down[3] = gpt2_pack_down(h.L, h.S, h.C, h.D); sh_down_nr[3] = nr8; }
    }
    __syncthreads();
    if (lane == 0) from_below = sh_up[wave];
    if (lane == 63) { from_above = sh_down[wave]; from_above_nr = sh_down_nr[wave]; }
    const Gpt2Halo hl = digits_take_left<INDIVIDUAL>(from_below, w, m, Nr);
    const Gpt2Halo hr = digits_take_right<INDIVIDUAL>(from_above, from_above_nr, w, n_bytes, spill);
    uint64_t ld = 0;
    const unsigned long long out = gpt2_word_starts(m, hl, hr, text, w, LEAD ? &ld : nullptr);
    if (w < n_words_host) {
        startmask[w] = out;
        if constexpr (LEAD) leadmask[w] = (unsigned long long)ld;
    }
}
