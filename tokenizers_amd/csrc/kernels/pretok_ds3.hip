// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after kernels/pretok_window.hip, whose
// helpers it calls, and kernels/pretok_llama3.hip, whose k_l3_slow_docs it shares; it is not compiled on its own).  The DeepSeek-V3 / R1
// chain of three Splits in front of ByteLevel(use_regex=false): per-lane kernel, sequential per-document matcher.  There is no tile tier.

// =================================================================================================
// K_pretok_ds3_lane: Sequence[Split(\p{N}{1,3}), Split([CJK class]+), Split(main pattern), ByteLevel(use_regex=false)], bit-parallel PER
// LANE in the form of k_pretok_llama3_lane: a lane owns 48 bytes inside a 64-byte window (8 bytes of context on each side, four 16-byte
// loads), deposits one-hot byte flags from a small LDS table into 64-bit masks -- ASCII never touches a class table -- and runs
// ds3_window_starts (pretok_ds3_core.hpp), the mask algebra tests/test_split_chain.py checks on the CPU against the reference.  Bytes
// whose run leaves the window are reported in slowmask; k_l3_slow_docs lists their sentences for k_pretok_ds3_slow.
// LEAD: the lead-byte mask of the same text rides along (char offsets over a text read as it came: kernels/pretok_gpt2.hip)
// =================================================================================================
template <bool LEAD>
__global__ __launch_bounds__(256) void k_pretok_ds3_lane(const uint8_t* __restrict__ text, int64_t n_bytes_host,
                                                         const int64_t* __restrict__ len_dev,
                                                         const unsigned long long* __restrict__ docmask,
                                                         const uint16_t* __restrict__ uc1, const uint8_t* __restrict__ uc2,
                                                         const uint16_t* __restrict__ ps1, const uint8_t* __restrict__ ps2,
                                                         unsigned long long* __restrict__ startmask,
                                                         unsigned long long* __restrict__ slowmask, unsigned long long* __restrict__ leadmask) {
    __shared__ uint2 lut[SQ_LUT_COPIES * 256];
    {
        const L3Flags f = ds3_byte_flags(threadIdx.x);
#pragma unroll
        for (int c = 0; c < SQ_LUT_COPIES; ++c) lut[c * 256 + threadIdx.x] = make_uint2(f.x, f.y);
    }
    __syncthreads();
    const int64_t n_bytes = len_dev ? *len_dev : n_bytes_host;
    const int64_t n_words_host = (n_bytes_host >> 6) + 1;
    const int64_t Lg = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t a = Lg * L3W_MAIN;                         // first byte this lane decides
    const int64_t base = a - L3W_HALO;                       // window = [base, base + 64), 8-byte aligned
    unsigned long long st = 0, un = 0, ld = 0;
    if (a < n_bytes) {
        uint32_t w[16];
        window_load(text, base, w);
        L3Window m;
        window_valid(base, n_bytes, n_words_host, docmask, L3W_HALO, m.V, m.D);
        const uint2* my_lut = lut + (threadIdx.x & (SQ_LUT_COPIES - 1)) * 256;
        m.L = m.N = m.W = m.R = m.SP = m.C = m.AP = m.MU = 0;
        m.B5 = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            uint32_t accA = 0, accB = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 8 * g + j;
                const uint2 e = my_lut[(w[k >> 2] >> (8 * (k & 3))) & 0xFFu];
                accA |= e.x << j;
                accB |= e.y << j;
            }
            m.L |= (unsigned long long)(accA & 0xFFu) << (8 * g);
            m.N |= (unsigned long long)((accA >> 8) & 0xFFu) << (8 * g);
            m.W |= (unsigned long long)((accA >> 16) & 0xFFu) << (8 * g);
            m.R |= (unsigned long long)(accA >> 24) << (8 * g);
            m.SP |= (unsigned long long)(accB & 0xFFu) << (8 * g);
            m.C |= (unsigned long long)((accB >> 8) & 0xFFu) << (8 * g);
            m.AP |= (unsigned long long)((accB >> 16) & 0xFFu) << (8 * g);
            m.MU |= (unsigned long long)(accB >> 24) << (8 * g);
        }
        m.L &= m.V; m.N &= m.V; m.W &= m.V; m.R &= m.V; m.SP &= m.V; m.C &= m.V; m.AP &= m.V; m.MU &= m.V;
        if constexpr (LEAD) ld = ((m.V & ~m.C) >> L3W_HALO) & ((1ull << L3W_MAIN) - 1ull);
        uint64_t s64, u64;
        ds3_window_starts(m, text, base, uc1, uc2, ps1, ps2, &s64, &u64);
        st = (s64 >> L3W_HALO) & ((1ull << L3W_MAIN) - 1ull);
        un = (u64 >> L3W_HALO) & ((1ull << L3W_MAIN) - 1ull);
    }
    // four lanes' 48-bit results are three 64-bit mask words
    const unsigned long long st_n = __shfl_down(st, 1, 64), un_n = __shfl_down(un, 1, 64);
    const int q = (int)(threadIdx.x & 3);
    if (q < 3) {
        const int64_t word = 3 * (Lg >> 2) + q;
        if (word < n_words_host) {
            startmask[word] = (st >> (16 * q)) | (st_n << (L3W_MAIN - 16 * q));
            slowmask[word] = (un >> (16 * q)) | (un_n << (L3W_MAIN - 16 * q));
        }
    }
    if constexpr (LEAD) {
        const unsigned long long ld_n = __shfl_down(ld, 1, 64);
        if (q < 3) {
            const int64_t word = 3 * (Lg >> 2) + q;
            if (word < n_words_host) leadmask[word] = (ld >> (16 * q)) | (ld_n << (L3W_MAIN - 16 * q));
        }
    }
}

// Slow path: the sentences (documents, or the pieces between added-token matches) in which the lane kernel left a byte undecided are
// matched sequentially -- ds3_doc_starts, exact for any run length -- one lane per sentence; the sentence's bits of the start mask are
// rewritten.
__global__ void k_pretok_ds3_slow(const uint8_t* __restrict__ text, const int64_t* __restrict__ doc_off,
                                  const uint32_t* __restrict__ slow_docs, const uint32_t* __restrict__ n_slow_docs,
                                  Ds3Seq q, unsigned long long* __restrict__ startmask) {
    const uint32_t n = *n_slow_docs;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t d = slow_docs[i];
        const int64_t a = doc_off[d], b = doc_off[d + 1];
        // clear the sentence's bits, then set one bit per pre-token start
        for (int64_t w = a >> 6; w <= (b - 1) >> 6; ++w) {
            int64_t lo = w << 6, hi = lo + 64;
            unsigned long long m = ~0ull;
            if (a > lo) m &= ~0ull << (a - lo);
            if (b < hi) m &= ~0ull >> (hi - b);
            atomicAnd(&startmask[w], ~m);
        }
        ds3_doc_starts(q, text + a, b - a, [&](int64_t p) {
            const int64_t g = a + p;
            atomicOr(&startmask[g >> 6], 1ull << (g & 63));
        });
    }
}
