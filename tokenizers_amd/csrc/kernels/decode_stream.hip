// Part of kernels.hip (ONE translation unit: this file is #included there, inside namespace tkamd, after the shared
// helpers; it is not compiled on its own).  Streaming decode.

// =================================================================================================
// DecodeStream (tokenizer/mod.rs step_decode_stream) for n_streams running sequences at once: one new id per stream and step in, the text
// that just became printable out.  The reference keeps, per stream, the window of ids, the text it has emitted for them (prefix) and
// the index a drain cuts at.  prefix is always the decode of the first `pe` ids of the window, so the state here is integers
// (kernels.hpp DsState) and a step is
//   push    the id joins the window (n0 -> n = n0 + 1 ids); the stream names three ranges of its window: [0, pe) -- the prefix --,
//           [0, n0) -- what the prefix becomes if it is empty -- and [0, n) -- the string of this step;
//   decode  the range decode of decode_batch, unchanged (capi/decode.cpp): first- and last-kept forms, CTC's dedup, ByteFallback's runs
//           and the lossy UTF-8 repair apply to a RANGE, which is what the reference does by decoding its window;
//   decide  steps 1 - 3 of the reference over the three decoded strings: lengths from their CSR, the last three bytes against U+FFFD,
//           starts_with as a byte compare; status and chunk length;
//   copy    behind the u32 scan of the chunk lengths: the chunk bytes, their CSR, and the drain (the window shifted down by pi).
// One lane per stream throughout: a stream's work is a few ids and a few dozen bytes.
// A FUSED object (TKAMD_STREAM_FUSED) runs push, decode and decide as ONE kernel, k_ds_step_fused: a lane decodes the three ranges of its own
// window through the per-token device functions of kernels/decode.hip into scratch sized by a bound, so the step needs no count on the
// host and only enqueues (launch_ds_step_fused: 6 kernels).  Push and decide are device functions both shapes share.
// status (uint8 per stream): 0 stepped, nothing to emit; 1 chunk; 2 not stepped (inactive); 3 InvalidPrefix (the window keeps the id and
// nothing is drained, as the reference leaves it); 4 the window is full: the id did not fit, the stream stays so until it is reset.
// =================================================================================================
constexpr uint8_t DS_NOTHING = 0, DS_CHUNK = 1, DS_INACTIVE = 2, DS_INVALID_PREFIX = 3, DS_FULL = 4;

// the push of ONE stream: its status if it is not stepped (inactive, stuck), else DS_NOTHING with the id in the window, n0 = the ids the
// window held and pe = the ids its prefix is the decode of
template <bool WIDE>
__device__ __forceinline__ uint8_t ds_push_one(const DsState& z, int64_t s, const void* __restrict__ ids, const uint8_t* __restrict__ active, uint32_t& n0, uint32_t& pe) {
    n0 = z.n[s];
    pe = 0u;
    if (active && !active[s]) return DS_INACTIVE;
    if (z.stuck[s] || n0 >= z.window) { z.stuck[s] = 1; return DS_FULL; }
    uint32_t id;
    if (WIDE) {                                                // (as the range gather: a value that is no uint32 is an id no vocabulary has)
        const int64_t v = ((const int64_t*)ids)[s];
        id = (v < 0 || v > (int64_t)0xFFFFFFFFll) ? 0xFFFFFFFFu : (uint32_t)v;
    } else id = ((const uint32_t*)ids)[s];
    z.win[s * (int64_t)z.window + n0] = id;
    z.n[s] = n0 + 1u;
    pe = min(z.pe[s], n0);
    return DS_NOTHING;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_ds_push(DsState z, const void* __restrict__ ids, const uint8_t* __restrict__ active, int64_t* __restrict__ begin,
                                                 int64_t* __restrict__ end, uint8_t* __restrict__ status) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= z.n_streams) return;
    const int64_t base = s * (int64_t)z.window;
    int64_t e0 = base, e1 = base, e2 = base;                  // (a stream that is not stepped: three empty ranges)
    uint32_t n0, pe;
    const uint8_t stt = ds_push_one<WIDE>(z, s, ids, active, n0, pe);
    if (stt == DS_NOTHING) {
        e0 = base + pe;
        e1 = base + n0;
        e2 = base + n0 + 1;
    }
    int64_t* const b = begin + s * DS_RANGES;
    int64_t* const e = end + s * DS_RANGES;
    b[0] = b[1] = b[2] = base;
    e[0] = e0; e[1] = e1; e[2] = e2;
    status[s] = stt;
}
// str::ends_with('\u{FFFD}') of text[lo, hi)
__device__ __forceinline__ bool ds_ends_fffd(const uint8_t* text, int64_t lo, int64_t hi) {
    return hi - lo >= 3 && text[hi - 3] == 0xEFu && text[hi - 2] == 0xBFu && text[hi - 1] == 0xBDu;
}
// steps 1 - 3 of the reference for ONE stream that has pushed, over its three decoded strings -- the prefix text[p_lo, p_hi), the decode
// of the ids in front of the step text[q_lo, q_hi), the string of this step text[s_lo, s_hi) --: the status, and l = the chunk's length
__device__ __forceinline__ uint8_t ds_decide_one(const DsState& z, int64_t s, const uint8_t* text, int64_t p_lo, int64_t p_hi, int64_t q_lo, int64_t q_hi,
                                                 int64_t s_lo, int64_t s_hi, uint32_t& l) {
    const uint32_t n0 = z.n[s] - 1u;
    int64_t pre = p_lo, pre_len = p_hi - p_lo;
    l = 0u;
    // 1. an empty prefix in front of ids: it becomes their decode, unless that ends in a character still under way
    if (pre_len == 0 && n0 > 0u && !ds_ends_fffd(text, q_lo, q_hi)) {
        z.pe[s] = n0;
        z.pi[s] = n0;
        pre = q_lo;
        pre_len = q_hi - q_lo;
    }
    // 3. the string of this step against the prefix
    if (s_hi - s_lo > pre_len && !ds_ends_fffd(text, s_lo, s_hi)) {
        for (int64_t i = 0; i < pre_len; ++i)
            if (text[pre + i] != text[s_lo + i]) return DS_INVALID_PREFIX;
        l = (uint32_t)(s_hi - s_lo - pre_len);
        return DS_CHUNK;
    }
    return DS_NOTHING;
}
__global__ __launch_bounds__(256) void k_ds_decide(DsState z, uint8_t* __restrict__ status, const int64_t* __restrict__ doc_off, const uint8_t* __restrict__ text,
                                                   uint32_t* __restrict__ len) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= z.n_streams) return;
    uint32_t l = 0u;
    if (status[s] == DS_NOTHING) {
        const int64_t* const o = doc_off + s * DS_RANGES;
        const int64_t o0 = o[0], o1 = o[1], o2 = o[2], o3 = o[3];
        status[s] = ds_decide_one(z, s, text, o0, o1, o1, o2, o2, o3, l);
    }
    len[s] = l;
}
// The whole step in front of the scan, one lane a stream: the push, the three strings of its own window -- dec_lane_sequence, and behind
// it the lossy repair for ByteLevel: the rules of kernels/decode.hip, stated there alone -- into the stream's slot of f.scratch, the
// decision.  A slot is three strings of f.cap bytes (prefix | the ids in front of the step | the string of this step) and, for
// ByteLevel, a fourth for the text before its repair; f.cap >= window x the longest string an id can contribute, so no string outgrows
// its place (capi/decode_stream.cpp derives it).  str_end[s * DS_RANGES + 3] = where the step's string ends in f.scratch: the one entry
// k_ds_copy reads of a stream's CSR.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_ds_step_fused(DsState z, DsFused f, const void* __restrict__ ids, const uint8_t* __restrict__ active,
                                                       uint8_t* __restrict__ status, uint32_t* __restrict__ len, int64_t* __restrict__ str_end) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= z.n_streams) return;
    uint32_t n0, pe, l = 0u;
    uint8_t stt = ds_push_one<WIDE>(z, s, ids, active, n0, pe);
    int64_t s_hi = 0;
    if (stt == DS_NOTHING) {
        DecSeqView v;
        v.entry = (const uint4*)f.entry; v.blob = f.blob; v.n_ids = f.n_ids; v.skip_special = f.skip_special;
        v.position_forms = f.position_forms; v.from_end = f.from_end; v.byte_runs = f.byte_runs; v.dedup = f.dedup;
        const uint32_t* const win = z.win + s * (int64_t)z.window;
        uint8_t* const flag = f.flag + s * (int64_t)z.window;
        const int64_t slot = s * f.cap * (f.lossy ? 4 : 3);
        uint8_t* const raw = f.scratch + slot + 3 * f.cap;     // (ByteLevel only)
        auto decode = [&](uint32_t k, int64_t at) -> int64_t { // the decode of win[0, k) to f.scratch + at: where it ends
            if (!f.lossy) return at + dec_lane_sequence(v, win, k, flag, f.scratch + at);
            return at + lossy_lane_sequence(raw, dec_lane_sequence(v, win, k, flag, raw), f.scratch + at);
        };
        const int64_t p_lo = slot, p_hi = decode(pe, p_lo);
        int64_t q_lo = p_lo, q_hi = p_hi;                      // (pe == n0, as behind every drain: one range, one decode)
        if (pe != n0) { q_lo = slot + f.cap; q_hi = decode(n0, q_lo); }
        const int64_t s_lo = slot + 2 * f.cap;
        s_hi = decode(n0 + 1u, s_lo);
        stt = ds_decide_one(z, s, f.scratch, p_lo, p_hi, q_lo, q_hi, s_lo, s_hi, l);
    }
    status[s] = stt;
    len[s] = l;
    str_end[s * DS_RANGES + 3] = s_hi;
}
__global__ __launch_bounds__(256) void k_ds_copy(DsState z, const uint8_t* __restrict__ status, const int64_t* __restrict__ doc_off, const uint8_t* __restrict__ text,
                                                 const uint32_t* __restrict__ len, const uint32_t* __restrict__ pos, const int64_t* __restrict__ total,
                                                 uint8_t* __restrict__ out, int64_t* __restrict__ out_off) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > z.n_streams) return;
    if (s == z.n_streams) { out_off[s] = *total; return; }
    const uint32_t p = pos[s];
    out_off[s] = (int64_t)p;
    if (status[s] != DS_CHUNK) return;
    const uint32_t l = len[s];
    const uint8_t* const src = text + (doc_off[s * DS_RANGES + 3] - (int64_t)l);       // the tail of the step's string
    uint8_t* const dst = out + p;
    for (uint32_t i = 0; i < l; ++i) dst[i] = src[i];
    // the drain: ids[prefix_index..] stay, the prefix is the decode of all of them
    uint32_t* const win = z.win + s * (int64_t)z.window;
    const uint32_t n = z.n[s], cut = min(z.pi[s], n), left = n - cut;
    if (cut)
        for (uint32_t j = 0; j < left; ++j) win[j] = win[j + cut];
    z.n[s] = left;
    z.pe[s] = left;
    z.pi[s] = left;
}
__global__ __launch_bounds__(256) void k_ds_reset(DsState z, const int64_t* __restrict__ which, int64_t n_which) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_which) return;
    const int64_t s = which ? which[i] : i;
    if (s < 0 || s >= z.n_streams) return;                     // (the host has refused such a list)
    z.n[s] = 0u;
    z.pe[s] = 0u;
    z.pi[s] = 0u;
    z.stuck[s] = 0;
}
// one workgroup: the window of one stream becomes ids[0 .. n), n <= window
__global__ __launch_bounds__(256) void k_ds_seed(DsState z, int64_t s, const uint32_t* __restrict__ ids, uint32_t n) {
    uint32_t* const win = z.win + s * (int64_t)z.window;
    for (uint32_t j = threadIdx.x; j < n && j < z.window; j += 256u) win[j] = ids[j];
    if (threadIdx.x == 0) {
        z.n[s] = min(n, z.window);
        z.pe[s] = 0u;
        z.pi[s] = 0u;
        z.stuck[s] = 0;
    }
}
void launch_ds_push(hipStream_t st, const DsState& z, const void* ids, bool wide, const uint8_t* active, int64_t* begin, int64_t* end, uint8_t* status) {
    if (z.n_streams <= 0) return;
    const unsigned nb = blocks_for(z.n_streams, 256);
    if (wide) hipLaunchKernelGGL(k_ds_push<true>, dim3(nb), dim3(256), 0, st, z, ids, active, begin, end, status);
    else hipLaunchKernelGGL(k_ds_push<false>, dim3(nb), dim3(256), 0, st, z, ids, active, begin, end, status);
}
void launch_ds_emit(hipStream_t st, const DsState& z, uint8_t* status, const int64_t* doc_off, const uint8_t* text, uint32_t* len, uint32_t* bsum, uint32_t* pos,
                    int64_t* total, uint8_t* out, int64_t* out_off) {
    const int64_t S = z.n_streams;
    if (S > 0) {
        const unsigned nb = blocks_for(S, 256);
        hipLaunchKernelGGL(k_ds_decide, dim3(nb), dim3(256), 0, st, z, status, doc_off, text, len);
        hipLaunchKernelGGL(k_u32_reduce, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, S, bsum);
        hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, bsum, (int64_t)nb, (const int64_t*)nullptr, (int64_t)1, total);
        hipLaunchKernelGGL(k_u32_down, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, S, (const uint32_t*)bsum, pos);
    } else (void)hipMemsetAsync(total, 0, 8, st);
    hipLaunchKernelGGL(k_ds_copy, dim3(blocks_for(S + 1, 256)), dim3(256), 0, st, z, (const uint8_t*)status, doc_off, text, (const uint32_t*)len,
                       (const uint32_t*)pos, (const int64_t*)total, out, out_off);
    launch_decode_zero_pad(st, out, total);
}
// a fused step: 6 kernels (the step, the scan chain, the copy, the zero pad) whatever the decoder and whatever the windows hold; no
// streams: the memset, the copy (the CSR's one entry) and the pad
void launch_ds_step_fused(hipStream_t st, const DsState& z, const DsFused& f, const void* ids, bool wide, const uint8_t* active, uint8_t* status, uint32_t* len,
                          int64_t* str_end, uint32_t* bsum, uint32_t* pos, int64_t* total, uint8_t* out, int64_t* out_off) {
    const int64_t S = z.n_streams;
    if (S > 0) {
        const unsigned nb = blocks_for(S, 256);
        if (wide) hipLaunchKernelGGL(k_ds_step_fused<true>, dim3(nb), dim3(256), 0, st, z, f, ids, active, status, len, str_end);
        else hipLaunchKernelGGL(k_ds_step_fused<false>, dim3(nb), dim3(256), 0, st, z, f, ids, active, status, len, str_end);
        hipLaunchKernelGGL(k_u32_reduce, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, S, bsum);
        hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, bsum, (int64_t)nb, (const int64_t*)nullptr, (int64_t)1, total);
        hipLaunchKernelGGL(k_u32_down, dim3(nb), dim3(256), 0, st, (const uint32_t*)len, S, (const uint32_t*)bsum, pos);
    } else (void)hipMemsetAsync(total, 0, 8, st);
    hipLaunchKernelGGL(k_ds_copy, dim3(blocks_for(S + 1, 256)), dim3(256), 0, st, z, (const uint8_t*)status, (const int64_t*)str_end, (const uint8_t*)f.scratch,
                       (const uint32_t*)len, (const uint32_t*)pos, (const int64_t*)total, out, out_off);
    launch_decode_zero_pad(st, out, total);
}
void launch_ds_reset(hipStream_t st, const DsState& z, const int64_t* which, int64_t n_which) {
    const int64_t n = which ? n_which : z.n_streams;
    if (n > 0) hipLaunchKernelGGL(k_ds_reset, dim3(blocks_for(n, 256)), dim3(256), 0, st, z, which, n);
}
void launch_ds_seed(hipStream_t st, const DsState& z, int64_t stream, const uint32_t* ids, uint32_t n) {
    hipLaunchKernelGGL(k_ds_seed, dim3(1), dim3(256), 0, st, z, stream, ids, n);
}
