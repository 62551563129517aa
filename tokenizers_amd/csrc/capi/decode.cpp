// Part of capi.cpp (ONE translation unit: this file is #included there and is not compiled on its own): decode_batch.

// ---- decode_batch (tokenizer/mod.rs:1404-1416): ids CSR -> UTF-8 bytes CSR ----------------------------------------
int tkamd_decode_batch(tkamd_tokenizer* t, const uint32_t* ids, const int64_t* tok_offsets, int64_t n_docs, uint32_t flags,
                       tkamd_text** out) {
    if (!t || !out || !tok_offsets || n_docs < 0) return set_error(TKAMD_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (t->device < 0) return set_error(TKAMD_ERR_DEVICE, "host-only tokenizer handle: no HIP device bound (there is no CPU fallback)");
    return guarded([&]() -> int {
        const HostModel& hm = t->hm;
        if (hm.decoder == DEC_UNSUPPORTED) throw Unsupported("decode_batch: " + hm.dec_unsupported);
        check_not_forked();
        HIP_CHECK(hipSetDevice(t->device));
        HostLease lease(t);
        Workspace* w = lease.w;
        std::lock_guard<std::mutex> lk(w->mu);
        const int64_t n_tok = tok_offsets[n_docs];
        if (n_tok < 0 || tok_offsets[0] != 0) throw Invalid("tok_offsets is not a monotone CSR over [0, n_tokens]");
        for (int64_t d = 0; d < n_docs; ++d)
            if (tok_offsets[d + 1] < tok_offsets[d]) throw Invalid("tok_offsets is not monotone");
        if (n_tok > 0 && !ids) throw Invalid("null ids");
        if (n_tok >= ((int64_t)1 << 31)) throw Invalid("more than 2^31 tokens in one decode_batch call");
        hipStream_t st = own_stream(w);
        const uint32_t n_ids = (uint32_t)(hm.dec_entry.size() / 4);
        const size_t nb = (size_t)(n_tok / 256 + 2);
        w->dw_ids.reserve((size_t)n_tok * 4 + 64);
        w->dw_tok_off.reserve((size_t)(n_docs + 1) * 8);
        w->dw_first.reserve((size_t)(n_tok / 32 + 2) * 4);
        w->dw_len.reserve((size_t)n_tok * 4 + 64);
        w->dw_bsum.reserve(nb * 4);
        w->dw_pos.reserve((size_t)n_tok * 4 + 64);
        w->dw_out_off.reserve((size_t)(n_docs + 1) * 8);
        w->dw_total.reserve(64);
        if (n_tok) HIP_CHECK(hipMemcpyAsync(w->dw_ids.p, ids, (size_t)n_tok * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(w->dw_tok_off.p, tok_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st));
        uint32_t* firstmask = hm.dec_position_dependent ? w->dw_first.as<uint32_t>() : nullptr;
        uint32_t* badmask = nullptr;                          // ByteFallback: tokens of byte runs that are not UTF-8
        if (hm.dec_has_bytes) { w->dw_bad.reserve((size_t)(n_tok / 32 + 2) * 4); badmask = w->dw_bad.as<uint32_t>(); }
        uint32_t* dupmask = nullptr;                          // CTC: kept tokens equal to the kept token in front of them
        if (hm.dec_dedup) { w->dw_dup.reserve((size_t)(n_tok / 32 + 2) * 4); dupmask = w->dw_dup.as<uint32_t>(); }
        const uint32_t from_end = hm.dec_special_is_last ? 1u : 0u;
        const uint32_t skip = (flags & TKAMD_SKIP_SPECIAL) ? 1u : 0u;
        launch_decode(st, w->dw_ids.as<uint32_t>(), w->dw_tok_off.as<int64_t>(), n_docs, n_tok, t->t_dec_entry.p, n_ids, t->t_dec_blob.as<uint8_t>(), skip,
                      firstmask, w->dw_len.as<uint32_t>(), w->dw_bsum.as<uint32_t>(), w->dw_pos.as<uint32_t>(), w->dw_total.as<int64_t>(),
                      w->dw_out_off.as<int64_t>(), nullptr, from_end, badmask, dupmask);
        HIP_CHECK(hipGetLastError());
        int64_t total = 0;
        HIP_CHECK(hipMemcpyAsync(&total, w->dw_total.p, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (total >= ((int64_t)1 << 32)) throw Invalid("decoded text beyond 4 GiB in one decode_batch call");
        w->dw_bytes.reserve((size_t)total + 64);
        launch_decode(st, w->dw_ids.as<uint32_t>(), w->dw_tok_off.as<int64_t>(), n_docs, n_tok, t->t_dec_entry.p, n_ids, t->t_dec_blob.as<uint8_t>(), skip,
                      firstmask, w->dw_len.as<uint32_t>(), w->dw_bsum.as<uint32_t>(), w->dw_pos.as<uint32_t>(), w->dw_total.as<int64_t>(),
                      w->dw_out_off.as<int64_t>(), w->dw_bytes.as<uint8_t>(), from_end, badmask, dupmask);
        HIP_CHECK(hipGetLastError());
        std::unique_ptr<tkamd_text> b(new tkamd_text());
        b->n_docs = n_docs;
        b->n_bytes = total;
        b->bytes = pinned_get((size_t)total);
        b->doc_offsets = pinned_get((size_t)(n_docs + 1) * 8);
        if (total) HIP_CHECK(hipMemcpyAsync(b->bytes.p, w->dw_bytes.p, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(b->doc_offsets.p, w->dw_out_off.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        *out = b.release();
        return TKAMD_OK;
    });
}
// ---- decode_batch with the ids in HBM already and the text left there: the range gather in front of launch_decode's two phases, the lossy
// UTF-8 repair (ByteLevel) and the zero slack behind them (kernels/decode.hip).  On the caller's stream, in the workspace keyed by it. ----
// (the body: in workspace w, whose lock the caller holds, on the device the caller has set.  The public entry runs it in the workspace
// keyed by the stream; a decode stream -- capi/decode_stream.cpp -- in a workspace of its own, so that neither moves the other's text.)
static int decode_ranges_device(tkamd_tokenizer* t, Workspace* w, hipStream_t st, const void* d_ids, int64_t n_elems, const int64_t* d_begin, const int64_t* d_end,
                                int64_t n_docs, uint32_t flags, tkamd_device_text* out) {
    const HostModel& hm = t->hm;
    // 1. the ranges: lengths, their scan into the token CSR, the first range that is not inside [0, n_elems]
    const size_t nd = (size_t)n_docs + 1;
    w->dw_tok_off.reserve(nd * 8);
    w->dw_out_off.reserve(nd * 8);
    w->dw_rpos.reserve(nd * 4 + 64);
    w->dw_len.reserve(nd * 4 + 64);
    w->dw_bsum.reserve((nd / 256 + 2) * 4);
    w->dw_total.reserve(64);
    int64_t* scalars = w->dw_total.as<int64_t>();
    launch_decode_ranges(st, d_begin, d_end, n_docs, n_elems, w->dw_len.as<uint32_t>(), w->dw_bsum.as<uint32_t>(), w->dw_rpos.as<uint32_t>(),
                         w->dw_tok_off.as<int64_t>(), scalars);
    HIP_CHECK(hipGetLastError());
    int64_t head[3] = {0, 0, 0};                           // tokens by the u32 scan, the first bad range, tokens summed in 64 bits
    HIP_CHECK(hipMemcpyAsync(head, scalars + 1, 24, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (head[1]) {
        const int64_t d = n_docs - (head[1] >> 4);
        const int why = (int)(head[1] & 15);
        throw Invalid("decode_batch: sequence " + std::to_string(d) + (why & 1 ? ": begin > end" : why & 2 ? ": begin < 0" : why & 4 ? ": end > n_ids" : ": 2^31 ids or more"));
    }
    // (overlapping ranges can sum past 2^32 over a small array: the limit is held against the 64-bit sum, which the scan's total
    // equals below it)
    if (head[2] < 0 || head[2] >= ((int64_t)1 << 31)) throw Invalid("more than 2^31 tokens in one decode_batch call");
    const int64_t n_tok = head[0];
    if (n_tok != head[2]) throw std::runtime_error("decode_batch: the token scan and the token sum disagree");
    // 2. the ids, one lane each, into the array launch_decode reads; its first phase
    const uint32_t n_ids = (uint32_t)(hm.dec_entry.size() / 4);
    w->dw_ids.reserve((size_t)n_tok * 4 + 64);
    w->dw_first.reserve((size_t)(n_tok / 32 + 2) * 4);
    w->dw_len.reserve((size_t)n_tok * 4 + 64);
    w->dw_bsum.reserve((size_t)(n_tok / 256 + 2) * 4);
    w->dw_pos.reserve((size_t)n_tok * 4 + 64);
    launch_decode_gather(st, d_ids, (flags & TKAMD_DECODE_IDS_I64) != 0, d_begin, w->dw_rpos.as<uint32_t>(), n_docs, n_tok, w->dw_ids.as<uint32_t>());
    uint32_t* firstmask = hm.dec_position_dependent ? w->dw_first.as<uint32_t>() : nullptr;
    uint32_t* badmask = nullptr;
    if (hm.dec_has_bytes) { w->dw_bad.reserve((size_t)(n_tok / 32 + 2) * 4); badmask = w->dw_bad.as<uint32_t>(); }
    uint32_t* dupmask = nullptr;
    if (hm.dec_dedup) { w->dw_dup.reserve((size_t)(n_tok / 32 + 2) * 4); dupmask = w->dw_dup.as<uint32_t>(); }
    const uint32_t from_end = hm.dec_special_is_last ? 1u : 0u;
    const uint32_t skip = (flags & TKAMD_SKIP_SPECIAL) ? 1u : 0u;
    launch_decode(st, w->dw_ids.as<uint32_t>(), w->dw_tok_off.as<int64_t>(), n_docs, n_tok, t->t_dec_entry.p, n_ids, t->t_dec_blob.as<uint8_t>(), skip,
                  firstmask, w->dw_len.as<uint32_t>(), w->dw_bsum.as<uint32_t>(), w->dw_pos.as<uint32_t>(), scalars, w->dw_out_off.as<int64_t>(), nullptr,
                  from_end, badmask, dupmask);
    HIP_CHECK(hipGetLastError());
    int64_t total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, scalars, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (total >= ((int64_t)1 << 32)) throw Invalid("decoded text beyond 4 GiB in one decode_batch call");
    // 3. the bytes, and the zero slack an encode over them reads
    w->dw_bytes.reserve((size_t)total + TKAMD_TEXT_PAD + 16);
    launch_decode(st, w->dw_ids.as<uint32_t>(), w->dw_tok_off.as<int64_t>(), n_docs, n_tok, t->t_dec_entry.p, n_ids, t->t_dec_blob.as<uint8_t>(), skip,
                  firstmask, w->dw_len.as<uint32_t>(), w->dw_bsum.as<uint32_t>(), w->dw_pos.as<uint32_t>(), scalars, w->dw_out_off.as<int64_t>(),
                  w->dw_bytes.as<uint8_t>(), from_end, badmask, dupmask);
    launch_decode_zero_pad(st, w->dw_bytes.as<uint8_t>(), scalars);
    HIP_CHECK(hipGetLastError());
    out->d_bytes = w->dw_bytes.as<uint8_t>();
    out->d_doc_offsets = w->dw_out_off.as<int64_t>();
    out->d_n_bytes = scalars;
    out->n_bytes = total;
    // 4. String::from_utf8_lossy of the ByteLevel decoder: what the repaired text would hold and whether anything is to repair
    if (hm.decoder != DEC_BYTELEVEL || total == 0) return TKAMD_OK;
    launch_utf8_lossy_count(st, w->dw_bytes.as<uint8_t>(), total, w->dw_out_off.as<int64_t>(), n_docs, scalars);
    HIP_CHECK(hipGetLastError());
    int64_t fix[2] = {0, 0};                               // bytes of the repaired text, invalid subparts
    HIP_CHECK(hipMemcpyAsync(fix, scalars + 4, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (fix[1] == 0) return TKAMD_OK;
    if (fix[0] >= ((int64_t)1 << 32)) throw Invalid("decoded text beyond 4 GiB in one decode_batch call");
    w->dw_fixed.reserve((size_t)fix[0] + TKAMD_TEXT_PAD + 16);
    w->dw_len.reserve((size_t)total * 4 + 64);
    w->dw_bsum.reserve((size_t)(total / 256 + 2) * 4);
    w->dw_pos.reserve((size_t)total * 4 + 64);
    launch_utf8_lossy_repair(st, w->dw_bytes.as<uint8_t>(), total, w->dw_out_off.as<int64_t>(), n_docs, w->dw_len.as<uint32_t>(), w->dw_bsum.as<uint32_t>(),
                             w->dw_pos.as<uint32_t>(), scalars + 4, w->dw_fixed.as<uint8_t>());
    launch_decode_zero_pad(st, w->dw_fixed.as<uint8_t>(), scalars + 4);
    HIP_CHECK(hipGetLastError());
    out->d_bytes = w->dw_fixed.as<uint8_t>();
    out->d_n_bytes = scalars + 4;
    out->n_bytes = fix[0];
    return TKAMD_OK;
}
int tkamd_decode_batch_device(tkamd_tokenizer* t, const void* d_ids, int64_t n_elems, const int64_t* d_begin, const int64_t* d_end, int64_t n_docs,
                              uint32_t flags, void* hip_stream, tkamd_device_text* out) {
    if (!t || !out || n_docs < 0 || n_elems < 0 || (n_docs > 0 && (!d_begin || !d_end)) || (n_elems > 0 && !d_ids) || n_docs >= ((int64_t)1 << 31))
        return set_error(TKAMD_ERR_INVALID, "bad argument");
    *out = tkamd_device_text{};
    if (t->device < 0) return set_error(TKAMD_ERR_DEVICE, "host-only tokenizer handle: no HIP device bound (there is no CPU fallback)");
    return guarded([&]() -> int {
        if (t->hm.decoder == DEC_UNSUPPORTED) throw Unsupported("decode_batch: " + t->hm.dec_unsupported);
        check_not_forked();
        hipStream_t st = (hipStream_t)hip_stream;
        Workspace* w = workspace_of_stream(t, st, true);
        std::lock_guard<std::mutex> lk(w->mu);
        HIP_CHECK(hipSetDevice(t->device));
        return decode_ranges_device(t, w, st, d_ids, n_elems, d_begin, d_end, n_docs, flags, out);
    });
}
// a result of the call above copied to host memory: what a binding without a HIP runtime of its own (ctypes) reads it with
int tkamd_device_text_read(tkamd_tokenizer* t, const tkamd_device_text* text, int64_t n_docs, int64_t n_slack, void* hip_stream, uint8_t* bytes,
                           int64_t* doc_offsets, int64_t* n_bytes) {
    if (!t || !text || n_docs < 0 || n_slack < 0 || n_slack > TKAMD_TEXT_PAD || !text->d_bytes || !text->d_doc_offsets || !text->d_n_bytes)
        return set_error(TKAMD_ERR_INVALID, "bad argument");
    if (t->device < 0) return set_error(TKAMD_ERR_DEVICE, "host-only tokenizer handle: no HIP device bound (there is no CPU fallback)");
    return guarded([&]() -> int {
        check_not_forked();
        hipStream_t st = (hipStream_t)hip_stream;
        HIP_CHECK(hipSetDevice(t->device));
        int64_t have = text->n_bytes;
        if (have < 0 && bytes) {                               // (a fused stream step's text: the count is on the device alone; one more wait)
            HIP_CHECK(hipMemcpyAsync(&have, text->d_n_bytes, 8, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (have < 0) throw std::runtime_error("device text: a negative byte count");
        }
        if (bytes && have + n_slack > 0) HIP_CHECK(hipMemcpyAsync(bytes, text->d_bytes, (size_t)(have + n_slack), hipMemcpyDeviceToHost, st));
        if (doc_offsets) HIP_CHECK(hipMemcpyAsync(doc_offsets, text->d_doc_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, st));
        if (n_bytes) HIP_CHECK(hipMemcpyAsync(n_bytes, text->d_n_bytes, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return TKAMD_OK;
    });
}
// from_utf8_lossy of ONE sequence by the host run of the core the kernels run (utf8_lossy_core.hpp)
int tkamd_probe_utf8_lossy(const uint8_t* bytes, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (n < 0 || (n > 0 && !bytes) || !n_out || cap < 0 || (cap > 0 && !out)) return set_error(TKAMD_ERR_INVALID, "bad argument");
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t l = utf8_lossy_len(bytes, i, 0, n);
        if (l == 1u) { if (k < cap) out[k] = bytes[i]; }
        else if (l == 3u && k + 3 <= cap) { out[k] = 0xEFu; out[k + 1] = 0xBFu; out[k + 2] = 0xBDu; }
        k += l;
    }
    *n_out = k;
    return k <= cap ? TKAMD_OK : set_error(TKAMD_ERR_INVALID, "output buffer too small");
}
int tkamd_decode_token(const tkamd_tokenizer* t, uint32_t id, int first_position, uint8_t* out, int32_t cap, int32_t* len, int32_t* flags) {
    if (!t || !len || !flags) return set_error(TKAMD_ERR_INVALID, "null argument");
    const HostModel& hm = t->hm;
    if (hm.decoder == DEC_UNSUPPORTED) return set_error(TKAMD_ERR_UNSUPPORTED, "decode_batch: " + hm.dec_unsupported);
    *len = 0;
    *flags = 2;                                              // absent
    if ((size_t)id * 4 + 3 >= hm.dec_entry.size()) return TKAMD_OK;
    const uint32_t* e = &hm.dec_entry[(size_t)id * 4];
    if (e[1] & DEC_ABSENT) return TKAMD_OK;
    *flags = (e[1] & DEC_SPECIAL) ? 1 : 0;
    if (e[1] & DEC_BYTE) {                                   // ByteFallback: the token's byte (what a run of them becomes is decided per run);
        *len = (int32_t)(first_position ? (e[1] & DEC_LEN_MASK) : e[3]);      // nothing as the first token under a leading Strip of this very byte
        if (*len && cap > 0 && out) out[0] = (uint8_t)e[0];
        return TKAMD_OK;
    }
    const uint32_t off = first_position ? e[0] : e[2], l = first_position ? (e[1] & DEC_LEN_MASK) : e[3];
    *len = (int32_t)l;
    for (uint32_t i = 0; i < l && (int32_t)i < cap && out; ++i) out[i] = hm.dec_blob[off + i];
    return TKAMD_OK;
}
