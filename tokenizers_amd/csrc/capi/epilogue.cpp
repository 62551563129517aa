// Part of capi.cpp (ONE translation unit: this file is #included there and is not compiled on its own): the epilogues of a batch (Batch, capi/pipeline.cpp) -- special tokens, truncation with its overflowing encodings, padding, pairs -- over the token CSR the stages left.

// PostProcessor::process for a single sequence (processors/bert.rs:51-120, template.rs:544-590): specials around every document
void Batch::add_specials() {
    const size_t T2 = (size_t)n_x + 4 + (size_t)(e_n + 1) * (hm.pp_prefix.size() + hm.pp_suffix.size());
    w->w_ids2.reserve(T2 * 4);
    w->w_tok_offsets2.reserve((size_t)(e_n + 2) * 8);
    if (out->d_offsets) w->w_offsets2.reserve(T2 * 8);
    if (out->d_word_ids) w->w_word_ids2.reserve(T2 * 4);
    SpecialArgs sa{};
    sa.tok_offsets = e_tok_off; sa.n_docs = e_n; sa.ids = w->w_ids.as<uint32_t>(); sa.offsets = out->d_offsets; sa.word_ids = out->d_word_ids;
    sa.prefix = t->t_pp_prefix.as<uint32_t>(); sa.suffix = t->t_pp_suffix.as<uint32_t>(); sa.n_prefix = (int32_t)hm.pp_prefix.size();
    sa.n_suffix = (int32_t)hm.pp_suffix.size(); sa.tok_offsets2 = w->w_tok_offsets2.as<int64_t>(); sa.ids2 = w->w_ids2.as<uint32_t>();
    sa.offsets2 = w->w_offsets2.as<uint32_t>(); sa.word_ids2 = w->w_word_ids2.as<uint32_t>(); sa.n_tok2 = sc + SC_NTOK2;
    pf.begin("add_specials");
    launch_add_specials(st, grid, sa);
    pf.end();
    publish_results(sa.ids2, (int64_t)T2, sa.tok_offsets2, sa.offsets2, sa.word_ids2, sa.n_tok2);
}

// BatchLongest (utils/padding.rs:55-63): the batch's longest encoding, read back from the device -- and, in a call that is sharded
// over several devices, exchanged with the other shards' (Workspace::pad_exchange), the batch's written back for the kernels behind.
// *again: a sharded call found its work queue too small -- the batch is run again BEFORE the exchange (every shard takes part in
// it exactly once; finish_batch's later re-run would hand in a second value the others no longer wait for).
uint64_t Batch::batch_longest(uint32_t* d_target, bool* again) {
    int64_t head[SC_PADMAX + 1];
    HIP_CHECK(hipMemcpyAsync(head, sc, sizeof(head), hipMemcpyDeviceToHost, st));
    uint32_t mx = 0;
    if (d_target != (uint32_t*)(sc + SC_PADMAX)) HIP_CHECK(hipMemcpyAsync(&mx, d_target, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (d_target == (uint32_t*)(sc + SC_PADMAX)) mx = *(const uint32_t*)&head[SC_PADMAX];
    if (!w->pad_exchange) return mx;
    if (rerun_wanted(t, w, *(const int*)&head[SC_ERR])) { *again = true; return 0; }
    const uint32_t all = w->pad_exchange(mx);
    if (all != mx) {
        w->h_padmax = all;
        HIP_CHECK(hipMemcpyAsync(d_target, &w->h_padmax, 4, hipMemcpyHostToDevice, st));
    }
    return all;
}

// The overflow epilogues' read-back of the scalars up to the number of encodings.  OVF_AGAIN: the token CSR is incomplete -- the call is
// synchronous here anyway, so the batch is run again right away (what finish_batch does for the calls that never wait).  OVF_ERROR: any
// other error -- the batch fails when it is synchronised; it is finished without the overflowing encodings.  Else the number of encodings.
enum : int64_t { OVF_AGAIN = -1, OVF_ERROR = -2 };
int64_t Batch::read_overflow_count(int64_t n_min) {
    int64_t head[SC_NENC + 1];
    HIP_CHECK(hipMemcpyAsync(head, sc, sizeof(head), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int raw = *(const int*)&head[SC_ERR];
    if (rerun_wanted(t, w, raw)) return OVF_AGAIN;
    if (raw & ~NOTE_BITS) return OVF_ERROR;
    if (head[SC_NENC] < n_min || head[SC_NENC] >= ((int64_t)1 << 31)) throw Invalid("the truncation leaves more than 2^31 overflowing encodings: raise max_length - stride or split the batch");
    return head[SC_NENC];
}

// Capacity of the padded arrays, from T2 = what the tokens and the special tokens need: known up front for Fixed; BatchLongest needs the batch
// maximum (one 4-byte read-back).  With overflowing encodings -- overlapping windows -- the token total is whatever the new CSR says: that CSR
// is built here (launch_final_offsets) and its total read back.  A sharded call with BatchLongest padding first takes the batch's longest
// encoding from the other shards (its value is not needed then: batch_longest wrote it back to the device target the kernels read).
size_t Batch::padded_capacity(const FinalArgs& fa, bool overflow, int64_t n_rows, size_t T2, const char* noun, bool* again) {
    if (overflow) {
        if (hm.pad_on && !hm.pad_fixed && w->pad_exchange) {
            (void)batch_longest(fa.target, again);
            if (*again) return 0;
        }
        launch_final_offsets(st, fa);
        int64_t total = 0;
        HIP_CHECK(hipMemcpyAsync(&total, fa.n_tok2, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (total < 0 || (uint64_t)total >= ((uint64_t)1 << 32))
            throw Invalid(std::string("the batch with its overflowing encodings would hold more than 2^32 tokens: encode fewer ") + noun + " per call");
        return (size_t)total + 4;
    }
    if (hm.pad_on) {
        uint64_t target = hm.pad_length;
        if (!hm.pad_fixed) {
            target = batch_longest(fa.target, again);
            if (*again) return 0;
        }
        if (hm.pad_multiple > 0 && target % hm.pad_multiple > 0) target += hm.pad_multiple - target % hm.pad_multiple;
        T2 += (size_t)n_rows * (size_t)target;
        if ((uint64_t)T2 >= ((uint64_t)1 << 32)) throw Invalid("the padded batch would hold more than 2^32 tokens: pad fewer documents per call");
    }
    return T2;
}

// The epilogue's arrays take the plain encodings' place in the result (n_enc >= 0: with the overflowing encodings).
void Batch::publish_results(uint32_t* ids2, int64_t capacity, int64_t* tok_offsets2, uint32_t* offsets2, uint32_t* word_ids2, int64_t* n_tok2, uint32_t* pad_count,
                            uint8_t* type_ids2, uint8_t* seq_ids2, int64_t n_enc, const uint32_t* enc_doc, const uint32_t* enc_idx) {
    if (n_enc >= 0) {
        w->last_n_enc = n_enc;
        out->d_enc_docs = enc_doc;
        out->d_enc_parts = enc_idx;
        out->d_n_encodings = sc + SC_NENC;
    }
    out->d_ids = ids2;
    out->ids_capacity = capacity;
    out->d_tok_offsets = tok_offsets2;
    if (out->d_offsets) out->d_offsets = offsets2;
    if (out->d_word_ids) out->d_word_ids = word_ids2;
    out->d_n_tokens = n_tok2;
    out->d_pad_counts = pad_count;
    out->d_type_ids = type_ids2;
    out->d_seq_ids = seq_ids2;
}

// EncodeInput::Dual: the two sequences of a pair were encoded as two documents; cut, lay out and pad them together
Step Batch::finalize_pairs() {
    const int64_t n_pairs = mixed ? n_inputs : e_n / 2;
    const bool tpl_on = (flags & TKAMD_ADD_SPECIAL) && !hm.pp_pair.empty();
    uint32_t n_special = 0;
    if (tpl_on) for (const HostModel::TplPiece& q : hm.pp_pair) n_special += q.kind == 2u;
    PairArgs pa{};
    pa.tok_offsets = e_tok_off; pa.n_pairs = n_pairs;
    if (mixed) {
        pa.inp_off = d_inp_off; pa.tpl1 = add_special ? t->t_pp_single.as<uint32_t>() : t->t_pp_single_plain.as<uint32_t>();
        pa.n_tpl1 = add_special ? (int32_t)hm.pp_single.size() : (int32_t)hm.pp_single_plain.size();
        pa.n_special1 = add_special ? (uint32_t)(hm.pp_prefix.size() + hm.pp_suffix.size()) : 0u;
    }
    const uint32_t n_special_max = std::max(n_special, pa.n_special1);      // (the bound of the output's size)
    pa.ids = w->w_ids.as<uint32_t>(); pa.offsets = out->d_offsets; pa.word_ids = out->d_word_ids; pa.trim1 = pa.offsets ? w->cur_trim1 : nullptr;
    w->w_keep.reserve((size_t)(std::max(e_n, 2 * n_pairs) + 2) * 4);
    pa.tpl = tpl_on ? t->t_pp_pair.as<uint32_t>() : t->t_pp_pair_plain.as<uint32_t>();
    pa.n_tpl = tpl_on ? (int32_t)hm.pp_pair.size() : (int32_t)hm.pp_pair_plain.size(); pa.n_special = n_special; pa.ovf_ty_tpl = (tpl_on && hm.pp_roberta) ? 1u : 0u;
    pa.trunc_on = hm.trunc_on ? 1u : 0u; pa.trunc_max = hm.trunc_max_length; pa.trunc_left = hm.trunc_left ? 1u : 0u;
    pa.trunc_strategy = (uint32_t)hm.trunc_strategy; pa.trunc_stride = hm.trunc_stride; pa.pad_on = hm.pad_on ? 1u : 0u; pa.pad_fixed = hm.pad_fixed ? 1u : 0u;
    pa.pad_length = hm.pad_length; pa.pad_multiple = hm.pad_multiple; pa.pad_left = hm.pad_left ? 1u : 0u; pa.pad_id = hm.pad_id; pa.pad_type_id = hm.pad_type_id;
    w->w_fbsum.reserve((size_t)((n_pairs + 1) / 256 + 2) * 4);
    pa.keep = w->w_keep.as<uint32_t>(); pa.bsum = w->w_fbsum.as<uint32_t>(); pa.target = (uint32_t*)(sc + SC_PADMAX); pa.n_tok2 = sc + SC_NTOK2; pa.err = d_err;
    for (int32_t k = 0; k < pa.n_tpl; ++k) {            // which sequence the template names first (it is "self" in the merge of the overflowing windows)
        const uint32_t kind = (tpl_on ? hm.pp_pair : hm.pp_pair_plain)[(size_t)k].kind;
        if (kind < 2u) { pa.first_is_b = kind == 1u ? 1u : 0u; break; }
    }
    pf.begin("pair_epilogue");
    int64_t n_enc = n_pairs;
    bool overflow = want_overflow;
    if (overflow) {
        w->w_ovf_parts.reserve((size_t)(n_pairs + 2) * 4);
        w->w_enc_base.reserve((size_t)(n_pairs + 2) * 8);
        pa.ovf_parts = w->w_ovf_parts.as<uint32_t>(); pa.enc_base = w->w_enc_base.as<int64_t>();
    } else {
        w->w_len1.reserve((size_t)(n_pairs + 2) * 4);
        pa.len1 = w->w_len1.as<uint32_t>();
    }
    launch_pair_lens(st, pa);
    if (overflow) {
        launch_pair_overflow_scan(st, pa, sc + SC_NENC);
        const int64_t got = read_overflow_count(n_pairs);
        if (got == OVF_AGAIN) { pf.end(); return Step::Again; }
        if (got == OVF_ERROR) {
            overflow = false;
            pa.ovf_parts = nullptr; pa.enc_base = nullptr;
            w->w_len1.reserve((size_t)(n_pairs + 2) * 4);
            pa.len1 = w->w_len1.as<uint32_t>();
            launch_pair_lens(st, pa);
        } else {
            n_enc = got;
            w->w_enc_doc.reserve((size_t)(n_enc + 2) * 4);
            w->w_enc_idx.reserve((size_t)(n_enc + 2) * 8);
            w->w_enc_win.reserve((size_t)(n_enc + 2) * 16);
            w->w_len1.reserve((size_t)(n_enc + 2) * 4);
            w->w_fbsum.reserve((size_t)((n_enc + 1) / 256 + 2) * 4);
            pa.enc_doc = w->w_enc_doc.as<uint32_t>(); pa.enc_idx = w->w_enc_idx.as<uint32_t>(); pa.enc_win = w->w_enc_win.as<uint32_t>();
            pa.len1 = w->w_len1.as<uint32_t>(); pa.bsum = w->w_fbsum.as<uint32_t>();
        }
    }
    w->w_fin.reserve((size_t)(n_enc + 2) * 4);
    w->w_tok_offsets2.reserve((size_t)(n_enc + 2) * 8);
    if (hm.pad_on) w->w_pad_count.reserve((size_t)(n_enc + 2) * 4);
    pa.fin = w->w_fin.as<uint32_t>(); pa.tok_offsets2 = w->w_tok_offsets2.as<int64_t>(); pa.pad_count = hm.pad_on ? w->w_pad_count.as<uint32_t>() : nullptr;
    if (overflow) launch_pair_ranges(st, pa);           // (pa.n_pairs still counts pairs)
    FinalArgs fa{};                                    // the CSR of the padded lengths: same three kernels as for single sequences
    fa.n_docs = n_enc;
    fa.len1 = pa.len1; fa.fin = pa.fin; fa.bsum = pa.bsum; fa.target = pa.target; fa.tok_offsets2 = pa.tok_offsets2; fa.n_tok2 = pa.n_tok2;
    fa.pad_on = pa.pad_on; fa.pad_fixed = pa.pad_fixed; fa.pad_length = pa.pad_length; fa.pad_multiple = pa.pad_multiple;
    bool again = false;
    const size_t T2 = padded_capacity(fa, overflow, n_pairs, (size_t)n_x + 4 + (size_t)(n_pairs + 1) * n_special_max, "pairs", &again);
    if (again) { pf.end(); return Step::Again; }
    w->w_ids2.reserve(T2 * 4);
    w->w_type_ids2.reserve(T2 + 64);
    w->w_seq_ids2.reserve(T2 + 64);
    if (out->d_offsets) w->w_offsets2.reserve(T2 * 8);
    if (out->d_word_ids) w->w_word_ids2.reserve(T2 * 4);
    pa.ids2 = w->w_ids2.as<uint32_t>(); pa.offsets2 = w->w_offsets2.as<uint32_t>(); pa.word_ids2 = w->w_word_ids2.as<uint32_t>();
    pa.type_ids2 = w->w_type_ids2.as<uint8_t>(); pa.seq_ids2 = w->w_seq_ids2.as<uint8_t>();
    if (!overflow) launch_final_offsets(st, fa);
    else pa.n_pairs = n_enc;                            // the copy runs per encoding
    launch_pair_finalize(st, grid, pa);
    pf.end();
    publish_results(pa.ids2, 0, pa.tok_offsets2, pa.offsets2, pa.word_ids2, pa.n_tok2, pa.pad_count, pa.type_ids2, pa.seq_ids2, overflow ? n_enc : -1, pa.enc_doc, pa.enc_idx);
    return Step::Done;
}

// truncation -> special tokens -> padding (tokenizer/mod.rs:1265-1317) as one epilogue over the token CSR
Step Batch::finalize() {
    const uint32_t n_add = add_special ? (uint32_t)(hm.pp_prefix.size() + hm.pp_suffix.size()) : 0u;
    FinalArgs fa{};
    fa.tok_offsets = e_tok_off; fa.n_docs = e_n; fa.ids = w->w_ids.as<uint32_t>(); fa.offsets = out->d_offsets; fa.word_ids = out->d_word_ids;
    fa.trim1 = fa.offsets ? w->cur_trim1 : nullptr; fa.prefix = t->t_pp_prefix.as<uint32_t>(); fa.suffix = t->t_pp_suffix.as<uint32_t>();
    fa.n_prefix = add_special ? (int32_t)hm.pp_prefix.size() : 0; fa.n_suffix = add_special ? (int32_t)hm.pp_suffix.size() : 0;
    // max_length - n_added_tokens when specials are added (mod.rs:1273-1279; the subtraction wraps in the reference's
    // release build when max_length is smaller: nothing is then truncated)
    fa.trunc_len = 0xFFFFFFFFu;
    if (hm.trunc_on) fa.trunc_len = (n_add && hm.trunc_max_length < n_add) ? 0xFFFFFFFFu : hm.trunc_max_length - n_add;
    fa.trunc_left = hm.trunc_left ? 1u : 0u; fa.trunc_needs_pair = (hm.trunc_on && hm.trunc_strategy == 2) ? 1u : 0u; fa.trunc_stride = hm.trunc_stride;
    fa.pad_on = hm.pad_on ? 1u : 0u; fa.pad_fixed = hm.pad_fixed ? 1u : 0u; fa.pad_length = hm.pad_length; fa.pad_multiple = hm.pad_multiple;
    fa.pad_left = hm.pad_left ? 1u : 0u; fa.pad_id = hm.pad_id;
    w->w_fbsum.reserve((size_t)((e_n + 1) / 256 + 2) * 4);
    fa.bsum = w->w_fbsum.as<uint32_t>(); fa.target = (uint32_t*)(sc + SC_PADMAX); fa.n_tok2 = sc + SC_NTOK2; fa.err = d_err;
    pf.begin("truncate_pad");
    int64_t n_enc = e_n;                                   // encodings of the result
    bool overflow = want_overflow;
    if (overflow) {
        // how many encodings every document leaves -> their numbering; the total is read back because everything below is
        // sized and launched per encoding
        w->w_ovf_parts.reserve((size_t)(e_n + 2) * 4);
        w->w_enc_base.reserve((size_t)(e_n + 2) * 8);
        fa.ovf_parts = w->w_ovf_parts.as<uint32_t>(); fa.enc_base = w->w_enc_base.as<int64_t>();
        launch_overflow_count(st, fa, sc + SC_NENC);
        const int64_t got = read_overflow_count(e_n);
        if (got == OVF_AGAIN) { pf.end(); return Step::Again; }
        if (got == OVF_ERROR) overflow = false;
        else n_enc = got;
    }
    if (overflow) {
        w->w_enc_doc.reserve((size_t)(n_enc + 2) * 4);
        w->w_enc_start.reserve((size_t)(n_enc + 2) * 4);
        w->w_enc_cnt.reserve((size_t)(n_enc + 2) * 4);
        fa.enc_doc = w->w_enc_doc.as<uint32_t>(); fa.enc_start = w->w_enc_start.as<uint32_t>(); fa.enc_cnt = w->w_enc_cnt.as<uint32_t>();
        w->w_fbsum.reserve((size_t)((n_enc + 1) / 256 + 2) * 4);
        fa.bsum = w->w_fbsum.as<uint32_t>();
    }
    w->w_len1.reserve((size_t)(n_enc + 2) * 4);
    w->w_fin.reserve((size_t)(n_enc + 2) * 4);
    w->w_tok_offsets2.reserve((size_t)(n_enc + 2) * 8);
    if (hm.pad_on) w->w_pad_count.reserve((size_t)(n_enc + 2) * 4);
    fa.len1 = w->w_len1.as<uint32_t>(); fa.fin = w->w_fin.as<uint32_t>(); fa.tok_offsets2 = w->w_tok_offsets2.as<int64_t>();
    fa.pad_count = hm.pad_on ? w->w_pad_count.as<uint32_t>() : nullptr;
    if (overflow) {
        launch_overflow_ranges(st, fa);                    // (fa.n_docs still counts documents)
        fa.n_docs = n_enc;
    } else {
        launch_final_lens(st, fa);
    }
    bool again = false;
    const size_t T2 = padded_capacity(fa, overflow, e_n, (size_t)n_x + 4 + (size_t)(e_n + 1) * n_add, "documents", &again);
    if (again) { pf.end(); return Step::Again; }
    w->w_ids2.reserve(T2 * 4);
    if (out->d_offsets) w->w_offsets2.reserve(T2 * 8);
    if (out->d_word_ids) w->w_word_ids2.reserve(T2 * 4);
    fa.ids2 = w->w_ids2.as<uint32_t>(); fa.offsets2 = w->w_offsets2.as<uint32_t>(); fa.word_ids2 = w->w_word_ids2.as<uint32_t>();
    if (typed_single) {
        w->w_type_ids2.reserve(T2 + 64);
        w->w_seq_ids2.reserve(T2 + 64);
        fa.type_ids2 = w->w_type_ids2.as<uint8_t>(); fa.seq_ids2 = w->w_seq_ids2.as<uint8_t>(); fa.prefix_ty = t->t_pp_prefix_ty.as<uint8_t>();
        fa.suffix_ty = t->t_pp_suffix_ty.as<uint8_t>(); fa.seq_ty = hm.pp_seq_ty; fa.pad_type_id = hm.pad_type_id;
    }
    if (!overflow) launch_final_offsets(st, fa);
    launch_finalize(st, grid, fa);
    pf.end();
    publish_results(fa.ids2, 0, fa.tok_offsets2, fa.offsets2, fa.word_ids2, fa.n_tok2, fa.pad_count, fa.type_ids2, fa.seq_ids2, overflow ? n_enc : -1, fa.enc_doc);
    return Step::Done;
}

// TKAMD_WANT_DENSE: the published result -> the caller's padded [n_rows, width] arrays (kernels/dense.hip).  check_request has settled
// that every row is `width` tokens long and that the arrays asked for have a source; the kernel reports a row that is not (ERR_INTERNAL).
void Batch::dense_rows() {
    const tkamd_dense_out& dd = w->last_dense;
    DenseArgs da{};
    da.tok_offsets = out->d_tok_offsets; da.ids = out->d_ids; da.pad_count = out->d_pad_counts; da.type_ids = out->d_type_ids; da.seq_ids = out->d_seq_ids;
    da.offsets = dd.offsets ? out->d_offsets : nullptr; da.word_ids = dd.word_ids ? out->d_word_ids : nullptr;
    da.input_ids = dd.input_ids; da.attention_mask = dd.attention_mask; da.token_type_ids = dd.token_type_ids; da.special_tokens_mask = dd.special_tokens_mask;
    da.offset_mapping = da.offsets ? dd.offsets : nullptr; da.out_word_ids = da.word_ids ? dd.word_ids : nullptr;
    da.n_rows = dd.n_rows; da.width = dd.width;
    da.pad_left = hm.pad_left ? 1u : 0u; da.n_prefix = add_special ? (uint32_t)hm.pp_prefix.size() : 0u; da.n_suffix = add_special ? (uint32_t)hm.pp_suffix.size() : 0u;
    da.pad_id = hm.pad_id; da.pad_type_id = hm.pad_type_id; da.err = d_err;
    pf.begin("dense_rows");
    launch_dense_rows(st, grid, da, (dd.dtype_flags & TKAMD_DENSE_I32) != 0);
    pf.end();
    out->ids_capacity = dd.n_rows * dd.width;
}

Step Batch::epilogue() {
    Step step = Step::Done;
    if (pairs) step = finalize_pairs();
    else if (has_epilogue) step = finalize();
    else if (add_special) add_specials();
    if (step == Step::Done) w->last_ntok_slot = (add_special || has_epilogue) ? SC_NTOK2 : SC_NTOK;
    if (step == Step::Done && want_dense) dense_rows();
    return step;
}
