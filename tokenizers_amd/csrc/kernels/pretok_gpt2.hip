// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers; it is not compiled on its own).  GPT-2 ByteLevel pre-tokenizer: the per-lane bit-parallel kernel (+ the class helpers the other
// pre-tokenizers share).  Rounds 1-2's lane-per-byte and ballot kernels are gone (round 6): HISTORY.md has their measurements.

// =================================================================================================
// The GPT-2 ByteLevel regex as a local-window predicate.
// Replaces: ByteLevel::pre_tokenize (pre_tokenizers/byte_level.rs:119-131) = Oniguruma find_iter
// over  's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+  (byte_level.rs:43-46)
// with SplitDelimiterBehavior::Isolated (normalizer.rs:694-783).  Every byte belongs to exactly one
// match, so the output is just "does a match start at byte i".  That predicate depends only on a
// window of <= 4 code points back / 3 ahead (verified against the reference):
//   con(i)  : a contraction literal matches at i AND i is itself a match start
//   eaten(i): i is a letter swallowed by a contraction
//   otherwise class-run rules with the " ?" optional-space attachment and the \s+(?!\S) lookahead.
// =================================================================================================
constexpr int PT_TILE = 2048;
constexpr int PT_HALO = 8;
constexpr int PT_R = PT_TILE + 2 * PT_HALO;

// info byte per text byte
constexpr uint32_t IF_CLS = 3;       // 0 other, 1 letter, 2 number, 3 whitespace
constexpr uint32_t IF_LEAD = 4;      // first byte of a code point
constexpr uint32_t IF_DOC = 8;       // first byte of a document
constexpr uint32_t IF_VALID = 16;    // inside [0, n_bytes)
constexpr uint32_t IF_SP = 32;       // U+0020
constexpr int IF_LEN_SHIFT = 6;      // (utf8 length - 1) in bits 6..7


__device__ __forceinline__ uint32_t cls_lns(uint32_t cp, const uint16_t* __restrict__ uc1, const uint8_t* __restrict__ uc2) {
    if (cp < 0x80u) {
        uint32_t lower = cp | 0x20u;
        if (lower - 'a' < 26u) return 1;
        if (cp - '0' < 10u) return 2;
        if (cp == 0x20u || cp - 9u < 5u) return 3;
        return 0;
    }
    uint32_t f = uc_flags(cp, uc1, uc2);
    return (f & UC_ONIG_L) ? 1u : (f & UC_ONIG_N) ? 2u : (f & UC_ONIG_S) ? 3u : 0u;
}

// decode the code point whose lead byte is sb[k]; sb must be readable to k+3
__device__ __forceinline__ uint32_t utf8_at(const uint8_t* sb, int k, uint32_t* len) {
    uint32_t b = sb[k];
    if (b < 0x80u) { *len = 1; return b; }
    if (b < 0xE0u) { *len = 2; return ((b & 0x1Fu) << 6) | (sb[k + 1] & 0x3Fu); }
    if (b < 0xF0u) { *len = 3; return ((b & 0x0Fu) << 12) | ((sb[k + 1] & 0x3Fu) << 6) | (sb[k + 2] & 0x3Fu); }
    *len = 4;
    return ((b & 0x07u) << 18) | ((sb[k + 1] & 0x3Fu) << 12) | ((sb[k + 2] & 0x3Fu) << 6) | (sb[k + 3] & 0x3Fu);
}

// =================================================================================================
// K_pretok_gpt2_seq: the GPT-2 start predicate, bit-parallel PER LANE, one lane per 64-bit word of the start mask.  A lane
// loads its own 64 bytes (four 16-byte loads) and classifies each of them exactly once: a byte indexes a small LDS table
// whose entries are one-hot flags spaced 8 bits apart (letter, digit, space-class, U+0020 | continuation, apostrophe,
// multi-byte lead), so ONE shift-or per byte deposits a flag into up to four masks at once and eight bytes later the
// finished groups move into 64-bit per-lane masks.  Multi-byte code points are resolved next (a short loop over their lead
// bits; what a code point puts on the next word is the lane's spill).  Then the neighbours: the regex looks at most four
// bytes ahead and three back, so a lane needs 8 bits of each mask of the word on either side -- one 64-bit word from the
// lane below (with its spill), one 32-bit word from the lane above.  Inside a wavefront they come by __shfl_up / __shfl_down,
// between the wavefronts of the workgroup through six words of LDS and one barrier, and at the two ends of the workgroup
// lanes 0 and 1 of the first wavefront classify the 8 bytes beyond it themselves (both in one pass of the same code): no
// workgroup waits for another.  The regex then is mask algebra on the vector ALU (pretok_gpt2_core.hpp gpt2_word_starts)
// and every lane stores its word.  The predicate: SURVEY Appendix A.1.
// (Until this form a lane decided the 48 bytes in the middle of a 64-byte window: every fourth byte was classified twice,
// the loads were 8-byte aligned, four lanes' results were shuffled into three words.)
// =================================================================================================
// SQ_LUT_COPIES: replicas of the per-lane kernels' 2 KB flag tables.  ONE since round 5: lanes that read the same entry are a broadcast,
// the same entry of two replicas is a bank conflict (four replicas: k_pretok_gpt2_seq 0.0521 -> 0.0495 ms, profiles/r5a_ab_c2.txt)
constexpr int SQ_MAIN = 48, SQ_HALO = 8, SQ_LUT_COPIES = 1;
struct __attribute__((packed, aligned(8))) SqChunk { uint32_t a, b, c, d; };
constexpr int G2_WORDS_PER_BLOCK = 256;      // k_pretok_gpt2_seq: one lane per mask word

// LEAD: the lead-byte mask of the same text rides along (char offsets over a text the pre-tokenizer reads as it came -- no normalizer, no
// prefix space: k_leadmask's pass over the same 120 MB, 0.025 ms, is not launched then).
template <int COPIES = SQ_LUT_COPIES, bool LEAD = false>
__global__ __launch_bounds__(256) void k_pretok_gpt2_seq(const uint8_t* __restrict__ text, int64_t n_bytes_host,
                                                         const int64_t* __restrict__ len_dev,
                                                         const unsigned long long* __restrict__ docmask,
                                                         const uint16_t* __restrict__ uc1, const uint8_t* __restrict__ uc2,
                                                         unsigned long long* __restrict__ startmask, unsigned long long* __restrict__ leadmask) {
    __shared__ Gpt2Flags lut[COPIES * 256];
    __shared__ unsigned long long sh_up[4];      // [v]: what the last lane of wavefront v - 1 hands up ([0]: the word in front of the workgroup)
    __shared__ uint32_t sh_down[4];              // [v]: what the first lane of wavefront v + 1 hands down ([3]: the word behind the workgroup)
    {
        const Gpt2Flags f = gpt2_byte_flags(threadIdx.x);    // 256 threads: one table entry each
#pragma unroll
        for (int c = 0; c < COPIES; ++c) lut[c * 256 + threadIdx.x] = f;
    }
    __syncthreads();
    const int64_t n_bytes = len_dev ? *len_dev : n_bytes_host;
    const int64_t n_words_host = (n_bytes_host >> 6) + 1;
    const int64_t w = (int64_t)blockIdx.x * G2_WORDS_PER_BLOCK + threadIdx.x;
    const Gpt2Flags* my_lut = lut + (threadIdx.x & (COPIES - 1)) * 256;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    // the word's own 64 bytes (a word past the text: all zero, no load)
    Gpt2Window m;
    const Gpt2Spill spill = gpt2_word_classify(text, n_bytes, (const uint64_t*)docmask, my_lut, w, uc1, uc2, m);
    const unsigned long long up = gpt2_pack_up(m, spill);
    const uint32_t down = gpt2_pack_down(m);
    unsigned long long from_below = __shfl_up(up, 1, 64);
    uint32_t from_above = __shfl_down(down, 1, 64);
    if (lane == 63 && wave < 3) sh_up[wave + 1] = up;
    if (lane == 0 && wave > 0) sh_down[wave - 1] = down;
    if (threadIdx.x < 2) {
        // the ends of the workgroup: thread 0 the 8 bytes in front of its own word, thread 1 the 8 bytes behind the workgroup's last word
        const int64_t pos = threadIdx.x == 0 ? (w << 6) - 8 : (w + G2_WORDS_PER_BLOCK - 1) << 6;
        const bool there = threadIdx.x == 0 ? (w > 0 && (w << 6) < n_bytes) : pos < n_bytes;
        Gpt2Halo h{0, 0, 0, 0, 0, 0, 0, 0};
        Gpt2Spill hs{0, 0, 0};
        if (there) h = gpt2_halo_classify(text, n_bytes, (const uint64_t*)docmask, my_lut, pos, uc1, uc2, &hs);
        if (threadIdx.x == 0) sh_up[0] = gpt2_pack_up(h.L, h.N, h.S, h.SP, h.AP, h.D, hs);
        else sh_down[3] = gpt2_pack_down(h.L, h.S, h.C, h.D);
    }
    __syncthreads();
    if (lane == 0) from_below = sh_up[wave];
    if (lane == 63) from_above = sh_down[wave];
    const Gpt2Halo hl = gpt2_take_left(from_below, w, m);
    const Gpt2Halo hr = gpt2_take_right(from_above, w, n_bytes, spill);
    uint64_t ld = 0;
    const unsigned long long out = gpt2_word_starts(m, hl, hr, text, w, LEAD ? &ld : nullptr);
    if (w < n_words_host) {
        startmask[w] = out;
        if constexpr (LEAD) leadmask[w] = (unsigned long long)ld;
    }
}
