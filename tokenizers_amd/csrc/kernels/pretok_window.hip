// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after kernels/pretok_gpt2.hip, whose
// SqChunk it loads with, and in front of the kernels that call it; it is not compiled on its own).  What the pre-tokenizer kernels that
// give one lane 48 bytes inside a 64-byte window share: k_pretok_llama3_lane, k_pretok_ds3_lane, k_pretok_local_lane.  The window's rule
// (pretok_{l3,ds3,local}_core.hpp) and which lanes have a window at all stay with each kernel.
// The flag-deposit loops and the "three mask words from four lanes" store stay written out in each kernel, and k_pretok_local_lane keeps
// its own V / D lines: see profiles/pretok_skeleton_isa.txt.

// the window's 64 bytes [base, base + 64) as 16 dwords: four 16-byte loads (8-byte aligned: gfx950 takes dwordx4 at any alignment); only
// lane 0's window starts before the text (base = -8)
__device__ __forceinline__ void window_load(const uint8_t* __restrict__ text, int64_t base, uint32_t (&w)[16]) {
    SqChunk c0{0u, 0u, 0u, 0u};
    if (base >= 0) c0 = *(const SqChunk*)(text + base);
    else { const uint2 t = *(const uint2*)text; c0.c = t.x; c0.d = t.y; }
    const SqChunk c1 = *(const SqChunk*)(text + base + 16), c2 = *(const SqChunk*)(text + base + 32), c3 = *(const SqChunk*)(text + base + 48);
    w[0] = c0.a; w[1] = c0.b; w[2] = c0.c; w[3] = c0.d; w[4] = c1.a; w[5] = c1.b; w[6] = c1.c; w[7] = c1.d;
    w[8] = c2.a; w[9] = c2.b; w[10] = c2.c; w[11] = c2.d; w[12] = c3.a; w[13] = c3.b; w[14] = c3.c; w[15] = c3.d;
}

// V: which bytes of the window exist; D: which of them start a document, gathered from two words of docmask (n_words_host words; not
// yet & V).  halo: the bytes of the window in front of the text when base < 0
__device__ __forceinline__ void window_valid(int64_t base, int64_t n_bytes, int64_t n_words_host, const unsigned long long* __restrict__ docmask,
                                             int halo, uint64_t& V, uint64_t& D) {
    const int vlo = base < 0 ? (int)-base : 0;
    const int64_t rem = n_bytes - base;
    V = (rem >= 64 ? ~0ull : ((1ull << rem) - 1ull)) & (~0ull << vlo);
    if (base < 0) D = docmask[0] << halo;
    else {
        const int64_t wi = base >> 6;
        const int sh = (int)(base & 63);
        D = docmask[wi] >> sh;
        if (sh && wi + 1 < n_words_host) D |= docmask[wi + 1] << (64 - sh);
    }
}
