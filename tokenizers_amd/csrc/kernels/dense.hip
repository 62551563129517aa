// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers; it is not compiled on its own).  The dense stage (TKAMD_WANT_DENSE): the published result of a batch -> the padded
// [n_rows, width] arrays a model reads, in memory the caller owns.

// =================================================================================================
// What transformers' BatchEncoding holds, written where the consumer wants it: input_ids, attention_mask, token_type_ids,
// special_tokens_mask, offset_mapping [n_rows, width, 2] and word_ids (-1: None), all int64 or all int32 (the template parameter).
// Every row of the published CSR is `width` tokens long -- truncation to <= width, Fixed padding to width: tkamd_dense_width -- with the
// pad ids and the special tokens already in it, so the stage is a widening copy plus the masks; dense_core.hpp decides every element.
//
// A streaming kernel: the outputs are taken as FLAT arrays of n_rows * width elements and a lane owns the 16 bytes that hold V = 2
// (int64) or 4 (int32) consecutive elements, wherever a row ends inside them -- consecutive lanes write consecutive 16-byte pieces
// whatever the width, and the stores are whole 16-byte ones for every width, odd ones included, where the array itself starts on a
// 16-byte boundary (else, and for the last few elements, element by element).  A row whose CSR length is not `width` cannot come out
// of the pipeline; it is still read inside its own [a, z) only, the columns it does not reach are written as padding, and the batch
// fails with ERR_INTERNAL.  All indices are int64: n_rows * width * 2 * 8 bytes pass 2^32.
// =================================================================================================
template <typename T, int V>
__device__ __forceinline__ void dense_store(void* base, bool wide, int64_t e0, int nv, const T* v) {
    T* const p = (T*)base + e0;
    if (wide && nv == V) {
        uint4 q;
        memcpy(&q, v, 16);
        *(uint4*)p = q;
    } else {
        for (int k = 0; k < nv; ++k) p[k] = v[k];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_dense_rows(DenseArgs a) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t total = a.n_rows * a.width;
    const int64_t n_groups = (total + V - 1) / V;
    const bool w_ids = ((uintptr_t)a.input_ids & 15u) == 0, w_att = ((uintptr_t)a.attention_mask & 15u) == 0, w_ty = ((uintptr_t)a.token_type_ids & 15u) == 0,
               w_sp = ((uintptr_t)a.special_tokens_mask & 15u) == 0, w_off = ((uintptr_t)a.offset_mapping & 15u) == 0, w_wid = ((uintptr_t)a.out_word_ids & 15u) == 0;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * 256) {
        const int64_t e0 = g * V;
        const int nv = (int)min((int64_t)V, total - e0);
        int64_t row = e0 / a.width, col = e0 - row * a.width;
        T v_ids[V], v_att[V], v_ty[V], v_sp[V], v_wid[V], v_off[2 * V];
        int64_t lo = 0, hi = 0;
        uint32_t pads = 0;
        bool fresh = true;                                  // the row changed: read its range
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v_ids[k] = v_att[k] = v_ty[k] = v_sp[k] = v_wid[k] = v_off[2 * k] = v_off[2 * k + 1] = 0;
            if (k >= nv) continue;
            if (fresh) {
                lo = a.tok_offsets[row];
                hi = a.tok_offsets[row + 1];
                pads = (a.pad_count && !a.seq_ids) ? a.pad_count[row] : 0u;
                if (hi - lo != a.width) atomicOr(a.err, ERR_INTERNAL);
                fresh = false;
            }
            const DenseSrc s = dense_element(lo, hi, pads, a.pad_left != 0u, a.n_prefix, a.n_suffix, a.width, col, a.seq_ids);
            const bool pad = s.kind == DENSE_PAD;
            v_ids[k] = (T)(s.src >= 0 ? a.ids[s.src] : a.pad_id);
            v_att[k] = pad ? 0 : 1;
            v_sp[k] = s.kind == DENSE_TOKEN ? 0 : 1;
            v_ty[k] = (T)((a.type_ids && s.src >= 0) ? (uint32_t)a.type_ids[s.src] : (pad ? a.pad_type_id : 0u));
            if (a.offset_mapping && s.src >= 0) {
                const uint2 o = *(const uint2*)(a.offsets + 2 * s.src);
                v_off[2 * k] = (T)o.x;
                v_off[2 * k + 1] = (T)o.y;
            }
            if (a.out_word_ids) {
                const uint32_t wd = s.src >= 0 ? a.word_ids[s.src] : 0xFFFFFFFFu;
                v_wid[k] = wd == 0xFFFFFFFFu ? (T)-1 : (T)wd;
            }
            if (++col == a.width) { col = 0; ++row; fresh = true; }
        }
        dense_store<T, V>(a.input_ids, w_ids, e0, nv, v_ids);
        if (a.attention_mask) dense_store<T, V>(a.attention_mask, w_att, e0, nv, v_att);
        if (a.token_type_ids) dense_store<T, V>(a.token_type_ids, w_ty, e0, nv, v_ty);
        if (a.special_tokens_mask) dense_store<T, V>(a.special_tokens_mask, w_sp, e0, nv, v_sp);
        if (a.out_word_ids) dense_store<T, V>(a.out_word_ids, w_wid, e0, nv, v_wid);
        if (a.offset_mapping) {                             // two elements a column: two 16-byte pieces a lane
            dense_store<T, V>(a.offset_mapping, w_off, 2 * e0, min(2 * nv, V), v_off);
            if (2 * nv > V) dense_store<T, V>(a.offset_mapping, w_off, 2 * e0 + V, 2 * nv - V, v_off + V);
        }
    }
}
