// Part of capi.cpp (ONE translation unit: this file is #included there and is not compiled on its own): DecodeStream for a batch of running sequences.

// ---- streaming decode (tokenizer/mod.rs step_decode_stream): n_streams DecodeStreams of one handle, state and text in HBM.  A step is
// push -> the range decode of decode_batch over three ranges a stream (decode_ranges_device, in a workspace of this object's own) ->
// decide / scan / copy (kernels/decode_stream.hip).  Nothing of a decoder is restated here or there.  A FUSED object (TKAMD_STREAM_FUSED)
// runs push, the three decodes and decide in one kernel over decode.hip's per-token device functions, in buffers sized at creation by a
// bound: its step only enqueues. ----
struct tkamd_decode_stream {
    tkamd_tokenizer* tok = nullptr;
    int device = 0;                      // tok->device (kept: the object may outlive a handle its owner has replaced, if only to be freed)
    int64_t n_streams = 0;
    uint32_t window = 32, skip = 0;
    std::mutex mu;                       // one call at a time
    Workspace ws;                        // what the range decode writes: its text is read by the step that asked for it and by nobody else
    DevBuf win, n, pe, pi, stuck;        // the state (kernels.hpp DsState)
    DevBuf begin, end, status, len, bsum, pos, out_off, total, chunk;      // a step's ranges and results
    // host lists on their way down (reset's indices, seed's ids, the ids and the mask of a step with TKAMD_STREAM_IDS_HOST): pinned, so the
    // copy is stream-ordered; `staged` says when the last one has left the block
    PinnedBlock stage;
    DevBuf stage_dev;
    size_t stage_cap = 0;
    hipEvent_t staged = nullptr;
    bool staged_pending = false;
    tkamd_device_text last{};            // the last step's result (tkamd_decode_stream_read); n_bytes < 0: the count is on the device alone so far
    bool has_last = false;
    // a fused object (TKAMD_STREAM_FUSED): everything a step touches, allocated at creation and sized by bounds (ds_fused_bound below)
    bool fused = false;
    DevBuf scratch, flag, str_end;       // kernels.hpp DsFused: a stream's decoded strings, its token masks; where its step's string ends
    int64_t longest = 0;                 // L: the most bytes one id contributes to a decoded string
    int64_t cap = 0;                     // bytes of one decoded string: window x max(L, 3), a multiple of 16
    int64_t chunk_capacity = 0, scratch_bytes = 0;
    DsFused view() const {
        const HostModel& hm = tok->hm;
        DsFused f;
        f.entry = tok->t_dec_entry.p; f.blob = tok->t_dec_blob.as<uint8_t>();
        f.n_ids = (uint32_t)(hm.dec_entry.size() / 4); f.skip_special = skip;
        f.position_forms = hm.dec_position_dependent ? 1u : 0u; f.from_end = hm.dec_special_is_last ? 1u : 0u;
        f.byte_runs = hm.dec_has_bytes ? 1u : 0u; f.dedup = hm.dec_dedup ? 1u : 0u; f.lossy = hm.decoder == DEC_BYTELEVEL ? 1u : 0u;
        f.scratch = scratch.as<uint8_t>(); f.flag = flag.as<uint8_t>(); f.cap = cap;
        return f;
    }
    DsState state() const {
        DsState z;
        z.win = win.as<uint32_t>(); z.n = n.as<uint32_t>(); z.pe = pe.as<uint32_t>(); z.pi = pi.as<uint32_t>(); z.stuck = stuck.as<uint8_t>();
        z.n_streams = n_streams; z.window = window;
        return z;
    }
    ~tkamd_decode_stream() {
        if (staged && !g_forked) (void)hipEventDestroy(staged);
        pinned_put(stage);
    }
};

// The bound a fused object is sized by.  A decoded string of k <= window ids is the concatenation of what its kept ids contribute:
//   * any decoder but ByteLevel: the id's string in one of its two position forms (dec_entry's lengths), or -- a <0xXX> token under
//     ByteFallback -- its byte, or U+FFFD, 3 bytes, when its run is not UTF-8: at most max(L, 3) bytes an id, L the longest form;
//   * ByteLevel: from_utf8_lossy runs over the concatenation.  A byte contributes 1 byte, 3 (it starts an invalid subpart) or none.
//     What the bytes of ONE id contribute together depends on the ids around it only at its edges, and never exceeds what they
//     contribute when the id stands alone: leading continuation bytes contribute 3 each alone, which is the most a byte can; a unit
//     that starts inside the id and ends inside it is decided inside it; a trailing lead with k < need well-formed continuation
//     bytes is ONE invalid subpart alone (3 bytes) and in company either completes (k + 1 <= 3 bytes, one each) or stays one subpart.
//     So L takes, for ByteLevel, the length of every form REPAIRED ALONE (>= the form's own length) -- GPT-2's longest token is ASCII
//     and both coincide.
// Hence a window's string, before and after the repair, is at most window x max(L, 3) bytes, and a chunk -- a tail of one -- as well.
static int64_t ds_longest_contribution(const HostModel& hm) {
    int64_t longest = 0;
    const size_t n_ids = hm.dec_entry.size() / 4;
    for (size_t id = 0; id < n_ids; ++id) {
        const uint32_t* e = &hm.dec_entry[id * 4];
        if (e[1] & DEC_ABSENT) continue;
        if (e[1] & DEC_BYTE) { longest = std::max<int64_t>(longest, 3); continue; }
        const uint32_t off[2] = {e[0], e[2]}, len[2] = {e[1] & DEC_LEN_MASK, e[3]};
        for (int f = 0; f < 2; ++f) {
            int64_t l = len[f];
            if (hm.decoder == DEC_BYTELEVEL) {
                l = 0;
                for (int64_t i = 0; i < (int64_t)len[f]; ++i) l += utf8_lossy_len(hm.dec_blob.data() + off[f], i, 0, (int64_t)len[f]);
                l = std::max<int64_t>(l, len[f]);
            }
            longest = std::max(longest, l);
            if (e[2] == e[0] && e[3] == len[0]) break;         // (one form)
        }
    }
    return longest;
}
constexpr int64_t DS_FUSED_LIMIT = (int64_t)1 << 30;       // bytes of strings and chunks a fused object may allocate

// `bytes` of host memory at `src` -> stage_dev + at, stream-ordered on st
static void ds_stage_down(tkamd_decode_stream* s, hipStream_t st, size_t at, const void* src, size_t bytes) {
    if (!bytes) return;
    memcpy((uint8_t*)s->stage.p + at, src, bytes);
    HIP_CHECK(hipMemcpyAsync(s->stage_dev.as<uint8_t>() + at, (const uint8_t*)s->stage.p + at, bytes, hipMemcpyHostToDevice, st));
}
static void ds_stage_begin(tkamd_decode_stream* s) {
    if (s->staged_pending) HIP_CHECK(hipEventSynchronize(s->staged));      // (the block's last copy has left it long ago, but for back-to-back resets)
    s->staged_pending = false;
}
static void ds_stage_end(tkamd_decode_stream* s, hipStream_t st) {
    HIP_CHECK(hipEventRecord(s->staged, st));
    s->staged_pending = true;
}

int tkamd_decode_stream_new(tkamd_tokenizer* t, int64_t n_streams, int32_t window, uint32_t flags, tkamd_decode_stream** out) {
    if (!t || !out || n_streams < 0 || n_streams >= ((int64_t)1 << 28)) return set_error(TKAMD_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (window == 0) window = 32;
    if (window < 2 || window > (1 << 20)) return set_error(TKAMD_ERR_INVALID, "decode_stream: the window holds at least 2 ids (and at most 2^20)");
    if (n_streams * (int64_t)window >= ((int64_t)1 << 31)) return set_error(TKAMD_ERR_INVALID, "decode_stream: 2^31 window slots or more");
    if (t->device < 0) return set_error(TKAMD_ERR_DEVICE, "host-only tokenizer handle: no HIP device bound (there is no CPU fallback)");
    return guarded([&]() -> int {
        if (t->hm.decoder == DEC_UNSUPPORTED) throw Unsupported("decode_batch: " + t->hm.dec_unsupported);
        check_not_forked();
        HIP_CHECK(hipSetDevice(t->device));
        std::unique_ptr<tkamd_decode_stream> s(new tkamd_decode_stream());
        s->tok = t;
        s->device = t->device;
        s->n_streams = n_streams;
        s->window = (uint32_t)window;
        s->skip = flags & TKAMD_SKIP_SPECIAL;
        s->fused = (flags & TKAMD_STREAM_FUSED) != 0;
        const size_t S = (size_t)n_streams;
        if (s->fused) {
            const bool lossy = t->hm.decoder == DEC_BYTELEVEL;
            s->longest = ds_longest_contribution(t->hm);
            const int64_t per_id = std::max<int64_t>(s->longest, 3);
            s->cap = ((int64_t)window * per_id + 15) / 16 * 16;                  // (window <= 2^20, a form < 2^29 bytes)
            const int64_t strings = lossy ? 4 : 3;
            // (compared by division: n_streams x cap x 5 stays far inside 64 bits, cap being at most the limit where it matters)
            if (s->cap > DS_FUSED_LIMIT || (n_streams > 0 && s->cap * (strings + 1) > DS_FUSED_LIMIT / n_streams))
                throw Invalid("decode_stream: a fused object of n_streams = " + std::to_string(n_streams) + ", window = " + std::to_string(window) + " and L = " +
                              std::to_string(s->longest) + " (the longest string one id decodes to) needs n_streams x window x max(L, 3) x " + std::to_string(strings + 1) +
                              " bytes, more than the limit of " + std::to_string(DS_FUSED_LIMIT));
            s->chunk_capacity = n_streams * s->cap;
            s->scratch_bytes = n_streams * s->cap * strings;
            s->scratch.reserve((size_t)s->scratch_bytes + 64);
            s->flag.reserve(S * (size_t)window + 64);
            s->str_end.reserve((S * DS_RANGES + 4) * 8);
            s->chunk.reserve((size_t)s->chunk_capacity + TKAMD_TEXT_PAD + 16);
        }
        s->win.reserve(S * (size_t)window * 4 + 64);
        s->n.reserve(S * 4 + 64);
        s->pe.reserve(S * 4 + 64);
        s->pi.reserve(S * 4 + 64);
        s->stuck.reserve(S + 64);
        s->begin.reserve(S * DS_RANGES * 8 + 64);
        s->end.reserve(S * DS_RANGES * 8 + 64);
        s->status.reserve(S + 64);
        s->len.reserve(S * 4 + 64);
        s->bsum.reserve((S / 256 + 2) * 4);
        s->pos.reserve(S * 4 + 64);
        s->out_off.reserve((S + 1) * 8);
        s->total.reserve(64);
        s->stage_cap = std::max(S * 9, (size_t)window * 4) + 64;
        s->stage_dev.reserve(s->stage_cap);
        s->stage = pinned_get(s->stage_cap);
        HIP_CHECK(hipEventCreateWithFlags(&s->staged, hipEventDisableTiming));
        // every stream empty, before any stream of the caller's can touch the state
        HIP_CHECK(hipMemset(s->n.p, 0, S * 4 + 64));
        HIP_CHECK(hipMemset(s->pe.p, 0, S * 4 + 64));
        HIP_CHECK(hipMemset(s->pi.p, 0, S * 4 + 64));
        HIP_CHECK(hipMemset(s->stuck.p, 0, S + 64));
        HIP_CHECK(hipDeviceSynchronize());
        *out = s.release();
        return TKAMD_OK;
    });
}
void tkamd_decode_stream_free(tkamd_decode_stream* s) {
    if (!s) return;
    if (g_forked) return;                // (inherited over fork(): the parent's device state is not ours to touch or free)
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
}
int tkamd_decode_stream_reset(tkamd_decode_stream* s, const int64_t* which, int64_t n, void* hip_stream) {
    if (!s || (which && (n < 0 || n > s->n_streams))) return set_error(TKAMD_ERR_INVALID, "bad argument");
    if (which)
        for (int64_t i = 0; i < n; ++i)
            if (which[i] < 0 || which[i] >= s->n_streams) return set_error(TKAMD_ERR_INVALID, "decode_stream: no stream " + std::to_string(which[i]));
    return guarded([&]() -> int {
        check_not_forked();
        std::lock_guard<std::mutex> lk(s->mu);
        HIP_CHECK(hipSetDevice(s->device));
        hipStream_t st = (hipStream_t)hip_stream;
        if (which && n > 0) {
            ds_stage_begin(s);
            ds_stage_down(s, st, 0, which, (size_t)n * 8);
            launch_ds_reset(st, s->state(), s->stage_dev.as<int64_t>(), n);
            ds_stage_end(s, st);
        } else if (!which) launch_ds_reset(st, s->state(), nullptr, 0);
        HIP_CHECK(hipGetLastError());
        return TKAMD_OK;
    });
}
int tkamd_decode_stream_seed(tkamd_decode_stream* s, int64_t which_one, const uint32_t* ids, int64_t n, void* hip_stream) {
    if (!s || n < 0 || (n > 0 && !ids)) return set_error(TKAMD_ERR_INVALID, "bad argument");
    if (which_one < 0 || which_one >= s->n_streams) return set_error(TKAMD_ERR_INVALID, "decode_stream: no stream " + std::to_string(which_one));
    if (n > (int64_t)s->window) return set_error(TKAMD_ERR_INVALID, "decode_stream: a seed of " + std::to_string(n) + " ids does not fit the window of " + std::to_string(s->window));
    return guarded([&]() -> int {
        check_not_forked();
        std::lock_guard<std::mutex> lk(s->mu);
        HIP_CHECK(hipSetDevice(s->device));
        hipStream_t st = (hipStream_t)hip_stream;
        ds_stage_begin(s);
        ds_stage_down(s, st, 0, ids, (size_t)n * 4);
        launch_ds_seed(st, s->state(), which_one, s->stage_dev.as<uint32_t>(), (uint32_t)n);
        ds_stage_end(s, st);
        HIP_CHECK(hipGetLastError());
        return TKAMD_OK;
    });
}
int tkamd_decode_stream_step(tkamd_decode_stream* s, const void* d_ids, const uint8_t* d_active, uint32_t flags, void* hip_stream, tkamd_device_text* text,
                             const uint8_t** d_status) {
    if (!s || !text || !d_status) return set_error(TKAMD_ERR_INVALID, "bad argument");
    *text = tkamd_device_text{};
    *d_status = nullptr;
    if (s->n_streams > 0 && !d_ids) return set_error(TKAMD_ERR_INVALID, "decode_stream: null ids");
    return guarded([&]() -> int {
        check_not_forked();
        std::lock_guard<std::mutex> lk(s->mu);
        tkamd_tokenizer* t = s->tok;
        HIP_CHECK(hipSetDevice(t->device));
        hipStream_t st = (hipStream_t)hip_stream;
        const int64_t S = s->n_streams;
        const bool wide = (flags & TKAMD_DECODE_IDS_I64) != 0;
        s->has_last = false;
        if ((flags & TKAMD_STREAM_IDS_HOST) && S > 0) {        // ids at 0, the mask behind the widest ids
            ds_stage_begin(s);
            ds_stage_down(s, st, 0, d_ids, (size_t)S * (wide ? 8 : 4));
            if (d_active) ds_stage_down(s, st, (size_t)S * 8, d_active, (size_t)S);
            ds_stage_end(s, st);
            d_ids = s->stage_dev.p;
            if (d_active) d_active = s->stage_dev.as<uint8_t>() + (size_t)S * 8;
        }
        const DsState z = s->state();
        if (s->fused) {                                        // enqueue only: every buffer was sized at creation, the count stays on the device
            int64_t* const total = s->total.as<int64_t>();
            launch_ds_step_fused(st, z, s->view(), d_ids, wide, d_active, s->status.as<uint8_t>(), s->len.as<uint32_t>(), s->str_end.as<int64_t>(),
                                 s->bsum.as<uint32_t>(), s->pos.as<uint32_t>(), total, s->chunk.as<uint8_t>(), s->out_off.as<int64_t>());
            HIP_CHECK(hipGetLastError());
            text->d_bytes = s->chunk.as<uint8_t>();
            text->d_doc_offsets = s->out_off.as<int64_t>();
            text->d_n_bytes = total;
            text->n_bytes = -1;
            *d_status = s->status.as<uint8_t>();
            s->last = *text;
            s->has_last = true;
            return TKAMD_OK;
        }
        launch_ds_push(st, z, d_ids, wide, d_active, s->begin.as<int64_t>(), s->end.as<int64_t>(), s->status.as<uint8_t>());
        HIP_CHECK(hipGetLastError());
        // the three ranges of every window through decode_batch's device entry, as it stands
        tkamd_device_text dec{};
        {
            std::lock_guard<std::mutex> wl(s->ws.mu);
            const int rc = decode_ranges_device(t, &s->ws, st, z.win, S * (int64_t)z.window, s->begin.as<int64_t>(), s->end.as<int64_t>(), S * DS_RANGES, s->skip, &dec);
            if (rc != TKAMD_OK) return rc;
        }
        // a chunk is a tail of a decoded string: the chunks together are no longer than the decoded text, whose size the host holds
        s->chunk.reserve((size_t)dec.n_bytes + TKAMD_TEXT_PAD + 16);
        int64_t* const total = s->total.as<int64_t>();
        launch_ds_emit(st, z, s->status.as<uint8_t>(), dec.d_doc_offsets, dec.d_bytes, s->len.as<uint32_t>(), s->bsum.as<uint32_t>(), s->pos.as<uint32_t>(), total,
                       s->chunk.as<uint8_t>(), s->out_off.as<int64_t>());
        HIP_CHECK(hipGetLastError());
        int64_t n_bytes = 0;
        HIP_CHECK(hipMemcpyAsync(&n_bytes, total, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (n_bytes < 0 || n_bytes > dec.n_bytes) throw std::runtime_error("decode_stream: the chunks are longer than the text they were cut from");
        text->d_bytes = s->chunk.as<uint8_t>();
        text->d_doc_offsets = s->out_off.as<int64_t>();
        text->d_n_bytes = total;
        text->n_bytes = n_bytes;
        *d_status = s->status.as<uint8_t>();
        s->last = *text;
        s->has_last = true;
        return TKAMD_OK;
    });
}
int tkamd_decode_stream_read(tkamd_decode_stream* s, int64_t n_slack, void* hip_stream, uint8_t* bytes, int64_t* doc_offsets, uint8_t* status) {
    if (!s || n_slack < 0 || n_slack > TKAMD_TEXT_PAD) return set_error(TKAMD_ERR_INVALID, "bad argument");
    return guarded([&]() -> int {
        check_not_forked();
        std::lock_guard<std::mutex> lk(s->mu);
        if (!s->has_last) throw Invalid("decode_stream: no step to read");
        HIP_CHECK(hipSetDevice(s->device));
        hipStream_t st = (hipStream_t)hip_stream;
        const int64_t S = s->n_streams;
        if (s->last.n_bytes < 0) {                             // a fused step: the count comes down first, with whatever does not need it
            int64_t n_bytes = 0;
            HIP_CHECK(hipMemcpyAsync(&n_bytes, s->last.d_n_bytes, 8, hipMemcpyDeviceToHost, st));
            if (doc_offsets) HIP_CHECK(hipMemcpyAsync(doc_offsets, s->last.d_doc_offsets, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, st));
            if (status && S > 0) HIP_CHECK(hipMemcpyAsync(status, s->status.p, (size_t)S, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (n_bytes < 0 || n_bytes > s->chunk_capacity) throw std::runtime_error("decode_stream: the chunks are longer than the bound they were sized by");
            // (not kept: a replayed graph refills these buffers without a call that could say so)
            if (bytes && n_bytes + n_slack > 0) {
                HIP_CHECK(hipMemcpyAsync(bytes, s->last.d_bytes, (size_t)(n_bytes + n_slack), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
            return TKAMD_OK;
        }
        if (bytes && s->last.n_bytes + n_slack > 0) HIP_CHECK(hipMemcpyAsync(bytes, s->last.d_bytes, (size_t)(s->last.n_bytes + n_slack), hipMemcpyDeviceToHost, st));
        if (doc_offsets) HIP_CHECK(hipMemcpyAsync(doc_offsets, s->last.d_doc_offsets, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, st));
        if (status && S > 0) HIP_CHECK(hipMemcpyAsync(status, s->status.p, (size_t)S, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return TKAMD_OK;
    });
}
int tkamd_decode_stream_peek(tkamd_decode_stream* s, int64_t which_one, uint32_t* ids, int64_t cap, int64_t* n, int64_t* pe, int64_t* pi) {
    if (!s || !n || !pe || !pi || cap < 0 || (cap > 0 && !ids)) return set_error(TKAMD_ERR_INVALID, "bad argument");
    if (which_one < 0 || which_one >= s->n_streams) return set_error(TKAMD_ERR_INVALID, "decode_stream: no stream " + std::to_string(which_one));
    return guarded([&]() -> int {
        check_not_forked();
        std::lock_guard<std::mutex> lk(s->mu);
        HIP_CHECK(hipSetDevice(s->device));
        HIP_CHECK(hipDeviceSynchronize());
        uint32_t v[3] = {0, 0, 0};
        HIP_CHECK(hipMemcpy(&v[0], s->n.as<uint32_t>() + which_one, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&v[1], s->pe.as<uint32_t>() + which_one, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&v[2], s->pi.as<uint32_t>() + which_one, 4, hipMemcpyDeviceToHost));
        *n = v[0]; *pe = v[1]; *pi = v[2];
        const int64_t k = std::min<int64_t>(std::min<int64_t>(cap, v[0]), s->window);
        if (k > 0) HIP_CHECK(hipMemcpy(ids, s->win.as<uint32_t>() + which_one * (int64_t)s->window, (size_t)k * 4, hipMemcpyDeviceToHost));
        return TKAMD_OK;
    });
}
int tkamd_decode_stream_info(tkamd_decode_stream* s, int64_t* fused, int64_t* chunk_capacity, int64_t* scratch_bytes) {
    if (!s) return set_error(TKAMD_ERR_INVALID, "bad argument");
    if (fused) *fused = s->fused ? 1 : 0;
    if (chunk_capacity) *chunk_capacity = s->chunk_capacity;
    if (scratch_bytes) *scratch_bytes = s->scratch_bytes;
    return TKAMD_OK;
}
