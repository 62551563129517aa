// Part of capi.cpp (ONE translation unit: this file is #included there and is not compiled on its own): the kernel sequence of one batch (run_pipeline and its stages), its queues and workspace sizes, the synchronisation and error mapping.

// Queue capacities for a text of N bytes.  Every queue is NSQ sub-queues (results.hip), one per lookup workgroup; a workgroup
// takes every grid-th tile of LOOKUP_TILE_BYTES.  A pre-token of class 1 / 2 / 3 is longer than 16 / 32 / 64 bytes, so those three
// are sized for the worst case outright; the <= 16-byte queue (worst case: half the bytes) starts at 1 / q16_div of them and
// the batch is run again with the worst-case size if it ever overflows (ERR_QUEUE_FULL; natural text queues 1/50 .. 1/6).
// the lookup's grid: what is resident at once (kernels/lookup.hip: three workgroups a CU), one private sub-queue per workgroup
int lookup_grid(const tkamd_tokenizer* t) { return std::min(3 * t->n_cu, (int)NSQ); }

struct QueueSizes {
    uint32_t sq_cap[4], row_base[4];
    size_t total;
};
// What the error word of a batch that has just been read back asks for besides failing: the batch again with a larger <= 16-byte queue
// (ERR_QUEUE_FULL alone), or again with the added tokens' matching passes (NOTE_ADDED_SEEN: it was run as if its text held none), or again
// through the NFC normalizer's kernels (NOTE_NFC_SEEN: it was run over the text as it came, and k_nfc_check cannot vouch for all of it).
static bool rerun_wanted(tkamd_tokenizer* t, Workspace* w, int raw) {
    const int err = raw & ~NOTE_BITS;
    bool again = false;
    if (raw & NOTE_ADDED_SEEN) { t->added_spec_pause = t->added_spec_len; w->force_general = true; again = true; }      // (force_general: the run that follows, whoever else draws on the pause)
    if (raw & NOTE_NFC_SEEN) { t->nfc_spec_pause = t->nfc_spec_len; w->force_nfc = true; ++t->nfc_reruns; again = true; }
    if (err == ERR_QUEUE_FULL && t->q16_div > 1) { t->q16_div = t->q16_div > 2 ? 2 : 1; again = true; }
    return again;
}

QueueSizes queue_sizes(size_t N, uint32_t q16_div, int grid) {
    QueueSizes z{};
    const size_t n_tiles = N / LOOKUP_TILE_BYTES + 1;
    const size_t per_sq = ((n_tiles + grid - 1) / grid) * LOOKUP_TILE_BYTES;
    z.sq_cap[0] = (uint32_t)(per_sq / q16_div + 64);
    z.sq_cap[1] = (uint32_t)(per_sq / 17 + 16);
    z.sq_cap[2] = (uint32_t)(per_sq / 33 + 16);
    z.sq_cap[3] = (uint32_t)(per_sq / 65 + 16);
    size_t acc = 0;
    for (int c = 0; c < 4; ++c) { z.row_base[c] = (uint32_t)acc; acc += (size_t)z.sq_cap[c] * (size_t)grid; }      // (sub-queues grid .. NSQ - 1 stay empty)
    z.total = acc;
    return z;
}

void reserve_workspace(tkamd_tokenizer* t, Workspace* w, int64_t n_bytes, int64_t n_docs, uint32_t flags, bool want_meta) {
    int64_t W = (n_bytes >> 6) + 2;
    size_t N = (size_t)n_bytes;
    w->w_docmask.reserve(W * 8);
    w->w_startmask.reserve(W * 8);
    w->w_wprefix.reserve(W * 4);
    w->w_bsum.reserve((W / 256 + 2) * 4);
    w->w_tok0.reserve((N + 4) * 4);
    w->w_tmp_ids.reserve((N + 4) * 4);
    const QueueSizes z = queue_sizes(N, t->q16_div, lookup_grid(t));
    w->w_rows.reserve(z.total * 16);
    w->w_queues.reserve(z.total * 8);
    w->w_cstate.reserve(lb_state_words(N / COMPACT_CHUNK + 4) * 8 + 16);
    w->w_chunk_lo.reserve((N / COMPACT_CHUNK + 4) * 4);
    w->w_qcount.reserve((size_t)QCNT_WORDS * 4);
    w->w_pt_tokoff.reserve((N + 4) * 4);
    w->w_ids.reserve((N + 4) * 4);
    w->w_doc_pt.reserve((n_docs + 2) * 4);
    w->w_tok_offsets.reserve((n_docs + 2) * 8);
    w->w_scalars.reserve(SC_SLOTS * 8);
    if (want_meta) w->w_pt_start.reserve((N + 4) * 4);      // pre-token offsets exist in memory only for the offsets / word-id pass
    if (flags & TKAMD_OFFSETS_MASK) {
        w->w_tmp_end.reserve((N + 4) * 4);
        w->w_offsets.reserve((N + 4) * 8);
    }
    if (flags & TKAMD_WANT_WORD_IDS) w->w_word_ids.reserve((N + 4) * 4);
}

using ull = unsigned long long;
// What the epilogue asks of run_pipeline: nothing more, or the batch again (its read-back found a work queue too small, or an added token in a
// text that was run as if it held none -- rerun_wanted).
enum class Step { Done, Again };

// One run of one batch: the call's arguments and the values decided for this run -- flags decoded, bounds, which text the kernels read, what
// the pre-tokenizer left behind.  Buffers stay in Workspace, tables in tkamd_tokenizer.  The stages are its member functions (their code reads
// the values by the names run_pipeline's locals had); run_pipeline calls them in order.
//
// Coordinate spaces: the ORIGINAL text (what the caller passed, what offsets refer to) and the X text
// (what the pre-tokenizer and the model read).  X == original unless a normalizer ran (BertNormalizer:
// bytes deleted/replaced, w_norig maps back) or ByteLevel add_prefix_space inserted leading spaces
// (documents shifted, mapped back per document).  When X is derived its length only exists on the
// device (x_len_dev); kernels are launched over the host-side bound n_x and read the effective length.
struct Batch {
    // the call (run_pipeline); d_doc_off / d_seq_off / d_inp_off become the validated copies in validate_inputs
    tkamd_tokenizer* t; Workspace* w; const uint8_t* d_text; const int64_t* d_doc_off; int64_t n_docs, n_bytes; const int64_t* d_seq_off; int64_t n_seqs;
    uint32_t flags; hipStream_t st; tkamd_device_result* out; const int64_t* d_inp_off; int64_t n_inputs;
    HostModel& hm = t->hm;
    Prof pf{t, w, st};
    // check_request
    bool mixed = false, want_words = false, want_meta = false, add_special = false, prefix_space = false, metaspace = false, words_in = false, pairs = false;
    bool typed_single = false, has_epilogue = false, want_overflow = false;
    bool want_dense = false;       // TKAMD_WANT_DENSE: the dense stage ends the epilogue (w->last_dense says where to)
    bool precomp = false;          // behind a Precompiled or an NFKC normalizer: the "▁" front reads its output (normalize_precompiled / normalize_nfkc)
    bool nfkc = false;             // ... the second of the two: normalized added tokens are matched over that output (pass 2)
    int64_t n_p = 0;               // ... the host's bound of that text
    const uint8_t* p_text = nullptr; const int64_t *p_doc_off = nullptr, *d_plen = nullptr; const uint32_t* p_norig = nullptr;
    bool nfc_general = false;      // behind an NFC normalizer: this run normalizes (else X is the text as it came, behind k_nfc_check)
    uint32_t off_mode = 0, mcap = 0;
    int64_t n_x = 0, e_n = 0, W0 = 0, W = 0;      // e_n: encodings the epilogues see; W0 / W: mask words over the original / the X text
    // zero_batch_state: the scalars' slots, the claims
    int64_t *sc = nullptr, *d_npretok = nullptr, *d_ntok_total = nullptr, *d_xlen = nullptr, *d_nseg = nullptr;
    uint32_t *d_counters = nullptr, *n_match = nullptr;
    int *d_err = nullptr, grid = 0;
    size_t claim_slots = 0;
    bool use_claims = false, lean = false;      // (lean: validate_inputs)
    const int64_t *raw_doc_off = nullptr, *e_tok_off = nullptr;      // e_tok_off: the token CSR the epilogues read (documents', or sequences of words')
    // build_x_text
    bool have_raw = false, have_norm = false, have_added = false;
    const ull* matchmask = nullptr;
    size_t seg_cap = 0, WX = 0;      // bound of the number of pieces between document / match edges; mask words covering either text
    const uint8_t* x_text = nullptr;
    const int64_t *x_doc_off = nullptr, *x_len_dev = nullptr, *piece_off = nullptr, *piece_n_dev = nullptr;
    const uint32_t *norig = nullptr, *norig_e = nullptr;
    int64_t n_in = 0;      // the text the second pass (and the prefix-space copy) reads
    // pretokenize
    bool lead_done = false;      // the pre-tokenizer wrote the lead-byte mask on its way (char offsets)
    bool has_end = false;        // the pre-tokenizer produced an end bitmask
    bool meta_masks = false;     // offsets / word ids: k_token_meta reads the pre-tokens' starts off the start mask (no pt_start array)
    uint32_t *mlist = nullptr, *tmp_end = nullptr, *pt_end = nullptr;  // pt_end: explicit pre-token ends in memory (offsets pass of the "Removed" pre-tokenizers)
    const uint32_t* pt_word = nullptr;
    WordCache wc{nullptr, nullptr, nullptr, 0u, nullptr};

    // the stages, in the order run_pipeline calls them (epilogue and what follows it: capi/epilogue.cpp)
    void check_request(); void zero_batch_state(); void validate_inputs(); void empty_batch();
    void build_x_text(); void pretokenize(); void run_model(); void compact_and_meta(); Step epilogue();
    // helpers of build_x_text
    AddedArgs args_of(int c);
    void scatter_masks(int64_t n_text, const int64_t* len_dev, bool with_end);
    const int64_t* build_pieces(const int64_t* doc_csr, int64_t n_text, const int64_t* len_dev);
    void normalize_bert(); void normalize_nfc(); void normalize_precompiled(); void normalize_nfkc(); void shift_behind_prefix_spaces(); void metaspace_front(); void read_ntext();
    // helpers of run_model / compact_and_meta
    void* phases_of(int which);
    void open_word_cache();
    void hot_census(const DevTables& lt, const ull* endmask);
    // the epilogues and what they share
    void add_specials(); Step finalize(); Step finalize_pairs(); void dense_rows();
    uint64_t batch_longest(uint32_t* d_target, bool* again);
    int64_t read_overflow_count(int64_t n_min);
    size_t padded_capacity(const FinalArgs& fa, bool overflow, int64_t n_rows, size_t T2, const char* noun, bool* again);
    void publish_results(uint32_t* ids2, int64_t capacity, int64_t* tok_offsets2, uint32_t* offsets2, uint32_t* word_ids2, int64_t* n_tok2, uint32_t* pad_count = nullptr,
                         uint8_t* type_ids2 = nullptr, uint8_t* seq_ids2 = nullptr, int64_t n_enc = -1, const uint32_t* enc_doc = nullptr, const uint32_t* enc_idx = nullptr);
};

// The row width a handle guarantees for dense output (tkamd_dense_width), or why it guarantees none: every encoding must come out of the
// epilogue exactly that long, and the caller must know the number before the call.
int64_t dense_width_of(const HostModel& hm, uint32_t flags) {
    if (!hm.trunc_on) throw Invalid("dense output needs a `truncation` section (enable_truncation): without one a row has no upper bound");
    if (!hm.pad_on) throw Invalid("dense output needs a `padding` section (enable_padding with a length)");
    if (!hm.pad_fixed) throw Invalid("dense output needs Fixed padding (enable_padding(length=...)): with BatchLongest the width is known on the device only");
    uint64_t width = hm.pad_length;
    if (hm.pad_multiple > 0 && width % hm.pad_multiple > 0) width += hm.pad_multiple - width % hm.pad_multiple;
    if (width < 1) throw Invalid("dense output: the padding length is 0");
    if ((uint64_t)hm.trunc_max_length > width)
        throw Invalid("dense output: truncation max_length " + std::to_string(hm.trunc_max_length) + " exceeds the padded width " + std::to_string(width) + ": rows would differ in length");
    if (flags & TKAMD_ADD_SPECIAL) {
        // (below the number of special tokens the reference's max_length - n_added_tokens wraps and nothing is cut: Batch::finalize)
        uint64_t n_add = hm.pp_prefix.size() + hm.pp_suffix.size();
        if (flags & TKAMD_PAIRS) {
            n_add = 0;
            for (const HostModel::TplPiece& q : hm.pp_pair) n_add += q.kind == 2u;
        }
        if ((uint64_t)hm.trunc_max_length < n_add)
            throw Invalid("dense output: truncation max_length " + std::to_string(hm.trunc_max_length) + " is below the " + std::to_string(n_add) +
                          " special tokens the template adds: nothing would be truncated");
    }
    return (int64_t)width;
}

// Decodes the flags and refuses what the build or the batch's size does not allow, in front of all device work.
void Batch::check_request() {
    mixed = n_inputs >= 0;
    if (mixed && (flags & TKAMD_PAIRS)) throw Invalid("a mixed batch names the kind of every input itself: TKAMD_PAIRS must not be set");
    if (mixed && !d_inp_off) throw Invalid("null input offsets");
    off_mode = flags & TKAMD_OFFSETS_MASK;
    want_words = (flags & TKAMD_WANT_WORD_IDS) != 0;
    want_meta = off_mode != TKAMD_OFFSETS_NONE || want_words;
    if (off_mode == 3u) throw Invalid("bad offsets mode");
    add_special = (flags & TKAMD_ADD_SPECIAL) != 0 && !(hm.pp_prefix.empty() && hm.pp_suffix.empty());
    if ((flags & TKAMD_ADD_SPECIAL) && !(flags & TKAMD_PAIRS) && !hm.pp_unsupported.empty()) throw Unsupported("add_special_tokens: " + hm.pp_unsupported);
    if (!(flags & TKAMD_PAIRS) && hm.pp_single_refused) throw Unsupported("post_processor: " + hm.pp_unsupported);
    if (mixed && (flags & TKAMD_ADD_SPECIAL) && !hm.pp_pair_unsupported.empty()) throw Unsupported("add_special_tokens on a pair: " + hm.pp_pair_unsupported);
    prefix_space = hm.byte_level && hm.add_prefix_space;
    metaspace = hm.pretok == PT_METASPACE;     // the "▁" front: X = the "▁" text (kernels/metaspace.hip)
    // host-side bound of the X text length: +1 per document for the virtual space; BertNormalizer can grow a
    // character (CJK spacing: 3 -> 5 bytes, NFD/lowercase expansions <= 3x) -- 3x the input covers every case
    // added-token matches of a batch: at most one per min_len bytes (the shortest pattern)
    size_t at_min_len = (size_t)-1;
    for (int c = 0; c < 2; ++c)
        for (size_t k = 0; k + 1 < hm.at[c].off.size(); ++k) at_min_len = std::min<size_t>(at_min_len, hm.at[c].off[k + 1] - hm.at[c].off[k]);
    const bool have_added_tokens = at_min_len != (size_t)-1;
    // (NFKC: every batch takes the normalizer's kernels -- no quick-check speculation yet, DESIGN section 8 -- and pass 2 runs over their output.
    // Matches do not overlap and each covers min_len bytes of the text it was found in, so the list is bounded by the longest text a pass
    // reads: behind NFKC the normalized text, up to NFK_GROWTH times the text as it came -- a token that occurs several times inside ONE
    // char's expansion, "\u0644" in that of U+FDFA, is more matches than the source has bytes.  The consumers of the list loop to the
    // count the matchers left, so the bound must hold; n_x and seg_cap below follow it.)
    nfkc = hm.norm == NORM_NFKC;
    const size_t match_text = nfkc ? (size_t)NFK_GROWTH * (size_t)n_bytes + 64 : (size_t)n_bytes;
    mcap = have_added_tokens ? (uint32_t)std::min<size_t>(match_text / std::max<size_t>(at_min_len, 1) + 16, 0x7FFFFFF0u) : 0u;
    // (a prefix space goes in front of every piece: every document, and what follows every match)
    // (the "▁" front: a ' ' becomes three bytes, and a "▁" of three goes in front of a piece -- every document, and what follows every match)
    // NFC: almost all text is NFC already, so a batch runs over the text as it came with k_nfc_check reading it once; one the check cannot
    // vouch for is run again through the normalizer (rerun_wanted), the handle's next nfc_spec_len batches normalize outright, and so does
    // every batch of a caller that never synchronises through the library (TKAMD_NO_SPECULATION).  (NFC grows UTF-8 text at most 3 x.)
    if (hm.norm == NORM_NFC) {
        nfc_general = w->force_nfc || (flags & TKAMD_NO_SPECULATION) || t->nfc_spec_len <= 0;
        w->force_nfc = false;
        if (!nfc_general) {
            int p = t->nfc_spec_pause.load();
            while (p > 0 && !t->nfc_spec_pause.compare_exchange_weak(p, p - 1)) {}
            nfc_general = p > 0;
        }
    }
    if (hm.nfd_mode()) nfc_general = true;          // (a chain that leaves NFD in the text: the normalizer's kernels for every batch, no quick check)
    // (Precompiled: a source byte stands for at most pc_growth output bytes, found at load; the "▁" front then reads that text)
    precomp = hm.norm == NORM_PRECOMPILED || nfkc;
    n_p = precomp ? (int64_t)(nfkc ? NFK_GROWTH : hm.pc_growth) * n_bytes + 64 : n_bytes;
    // (behind the normalizer only: every other tokenizer's text is bounded by the check of n_x below, as before)
    if (precomp && n_p >= (int64_t)0x55555500ll) throw Invalid("batch larger than 4 GiB behind the normalizer's bound: split it (byte offsets are 32-bit on the device)");
    n_x = (hm.norm == NORM_BERT || hm.norm == NORM_CHAIN || nfc_general) ? 3 * n_bytes + 64
          : metaspace ? 3 * n_p + 3 * (n_docs + 2 * (int64_t)mcap + 1) + 64
          : n_bytes + (prefix_space ? n_docs + (int64_t)mcap : 0);
    if (n_x >= (int64_t)0xFFFFFF00ll) throw Invalid("batch larger than 4 GiB: split it (byte offsets are 32-bit on the device)");
    const bool bpe_path = hm.model == MODEL_BPE && !hm.char_bpe && (hm.pretok == PT_BYTELEVEL_GPT2 || hm.pretok == PT_LLAMA3 || hm.pretok == PT_SPLIT_CHAIN || hm.pretok == PT_DIGITS_GPT2 ||
                                                                      hm.pretok == PT_BYTELEVEL_NOREGEX || hm.pretok == PT_CLIP || hm.pretok == PT_BLOOM);
    const bool local_pretok = hm.pretok == PT_WHITESPACE || hm.pretok == PT_WHITESPACE_SPLIT || hm.pretok == PT_BERT;
    const bool word_models = (hm.model == MODEL_WORDLEVEL || hm.model == MODEL_WORDPIECE) && local_pretok;
    const bool char_bpe = hm.model == MODEL_BPE && hm.char_bpe && (local_pretok || metaspace);      // BPE over characters rides the word models' pre-tokenizers, or the "▁" front
    const bool unigram = hm.model == MODEL_UNIGRAM && metaspace;                                     // Unigram: behind the "▁" front (split = true) only
    if (!bpe_path && !word_models && !char_bpe && !unigram)
        throw Unsupported("this build covers {ByteLevel(GPT-2 regex), Llama-3 Split+ByteLevel, ByteLevel(no regex)}+BPE and "
                          "{Whitespace,WhitespaceSplit,BertPreTokenizer}+{WordLevel,WordPiece,BPE over characters} and the U+2581 front+{BPE over characters, Unigram}");
    if (prefix_space && hm.norm != NORM_NONE) throw Unsupported("ByteLevel add_prefix_space behind a normalizer");
    // what the epilogues see: one encoding per document, or per sequence of words
    words_in = n_seqs >= 0;
    if (words_in && !d_seq_off) throw Invalid("null sequence offsets");
    e_n = words_in ? n_seqs : n_docs;
    pairs = (flags & TKAMD_PAIRS) != 0 || mixed;       // (a mixed batch: the pair epilogue lays out both kinds of input)
    if (pairs && !mixed && (e_n & 1)) throw Invalid("TKAMD_PAIRS: an odd number of documents");
    if (pairs && (flags & TKAMD_ADD_SPECIAL) && !hm.pp_pair_unsupported.empty()) throw Unsupported("add_special_tokens on a pair: " + hm.pp_pair_unsupported);
    typed_single = !pairs && hm.pp_single_typed;          // the single template's type ids: written by the epilogue, with or without special tokens
    has_epilogue = hm.trunc_on || hm.pad_on || pairs || typed_single;
    // Encoding.overflowing: what a truncation cuts off, as further encodings of the result (a pair leaves every combination of its two
    // sequences' windows, Encoding::merge_with encoding.rs:408-432)
    want_overflow = (flags & TKAMD_WANT_OVERFLOW) != 0 && hm.trunc_on;
    want_dense = (flags & TKAMD_WANT_DENSE) != 0;
    if (want_dense) {
        // everything the dense stage relies on is settled here, in front of all device work (the width's conditions: dense_width_of)
        if (!w->has_dense) throw Invalid("TKAMD_WANT_DENSE: only tkamd_encode_batch_device_dense takes this flag");
        const tkamd_dense_out& dd = w->last_dense;
        if (flags & TKAMD_WANT_OVERFLOW) throw Invalid("dense output with TKAMD_WANT_OVERFLOW: the number of rows would be known on the device only");
        if (words_in || mixed) throw Invalid("dense output of pre-tokenized or mixed inputs: these entries do not exist yet");
        if (!t->replicas.empty()) throw Invalid("dense output on a multi-device handle: the dense entry runs on one device, make a handle for it");
        if (!dd.input_ids) throw Invalid("dense output: input_ids is null");
        if (dd.dtype_flags & ~TKAMD_DENSE_I32) throw Invalid("dense output: unknown dtype_flags");
        if (dd.offsets && off_mode == TKAMD_OFFSETS_NONE) throw Invalid("dense output: offsets asked for without an offsets mode in flags (TKAMD_OFFSETS_BYTE / TKAMD_OFFSETS_CHAR)");
        if (dd.word_ids && !want_words) throw Invalid("dense output: word_ids asked for without TKAMD_WANT_WORD_IDS in flags");
        const int64_t width = dense_width_of(hm, flags), rows = pairs ? e_n / 2 : e_n;
        if (dd.n_rows != rows) throw Invalid("dense output: n_rows is " + std::to_string(dd.n_rows) + ", the batch has " + std::to_string(rows) + (pairs ? " pairs" : " documents"));
        if (dd.width != width) throw Invalid("dense output: width is " + std::to_string(dd.width) + ", tkamd_dense_width says " + std::to_string(width));
    }
    W0 = (n_bytes >> 6) + 1;
    W = (n_x >> 6) + 1;
    grid = t->n_cu * 8;
}

// Reserves the workspace, decides the claims and zeroes what the batch needs zeroed; the result starts as the plain encodings' arrays.
void Batch::zero_batch_state() {
    // (a device-entry caller holds the result pointers across a re-run: behind NFC the re-run's bound is the normalizer's, three times the
    // text, so its workspace is sized for that from the first run on -- grow-only buffers do not move then)
    reserve_workspace(t, w, (hm.norm == NORM_NFC && w->device_bound) ? 3 * n_bytes + 64 : n_x, n_docs, flags, want_meta);
    sc = w->w_scalars.as<int64_t>();
    d_npretok = sc + SC_NPRETOK;
    d_ntok_total = sc + SC_NTOK;
    d_xlen = sc + SC_NKEPT;
    d_err = (int*)(sc + SC_ERR);
    d_counters = (uint32_t*)(sc + SC_COUNTERS);
    // Everything the batch needs zeroed, in one launch: the scalars, the document mask, the queues' fill counters, the look-back state
    // of the compaction and the claims table (in-batch word claims, kernels/lookup.hip: on by default -- the test hook TKAMD_CLAIMS=0
    // switches them off, every occurrence of a word then goes to the model kernels; the word cache -- tkamd_word_cache, across batches --
    // takes their place when it is switched on).
    const char* const claims_hook = test_hook("TKAMD_CLAIMS");
    const bool claims_on = !(claims_hook && !strcmp(claims_hook, "0"));
    use_claims = claims_on && !t->word_cache &&
                 (hm.model == MODEL_BPE || hm.model == MODEL_UNIGRAM || (hm.model == MODEL_WORDPIECE && hm.max_input_chars >= (uint32_t)WORD_MAX_KEY));
    if (use_claims) {                                      // paused by an earlier batch that shared nothing (read_scalars)? one batch less to go
        int p = t->claims_pause.load();
        while (p > 0 && !t->claims_pause.compare_exchange_weak(p, p - 1)) {}
        if (p > 0) use_claims = false;
    }
    w->last_used_claims = use_claims;
    const size_t cstate_bytes = (lb_state_words((size_t)n_x / (size_t)COMPACT_CHUNK + 4) * 8 + 15) & ~(size_t)15;      // (the chunks' words and the groups')
    ZeroRegions z{};
    z.add(sc, SC_SLOTS * 8);
    // (behind BertNormalizer the mask covers the bound of the normalised text, three times the input: the words that text really has
    // are zeroed behind the normaliser, next to the slack of the text -- launch_zero_tail below)
    // (behind NFC's general path the whole bound is zeroed all the same: the byte-level pre-tokenizers walk the mask words of the bound, and that path is the rare one)
    if (!(hm.norm == NORM_BERT || (hm.norm == NORM_CHAIN && !hm.nfd_mode()) || metaspace)) z.add(w->w_docmask.p, (size_t)(W + 1) * 8);
    z.add(w->w_qcount.p, (size_t)QCNT_WORDS * 4);
    z.add(w->w_cstate.p, cstate_bytes);
    if (hm.pretok == PT_LLAMA3 && split_rule_fast(hm.split_rule)) {
        w->w_l3_tiles.reserve(l3_tileflag_words(n_x) * 8);
        z.add(w->w_l3_tiles.p, l3_tileflag_words(n_x) * 8);
    }
    if (use_claims) {
        // one slot per 64 bytes of the INPUT text (a word is a few bytes, most are repeats), 2^18 .. 2^24 slots: 32 MB of claims (two
        // 64-bit words a slot) + 32 MB of rows for a 120 MB batch.  (Not of the normalised text's bound, three times that behind BertNormalizer: the
        // words are the input's, and a table four times the size is four times the zeroing and a quarter of the cache hits.)
        // (a smaller table is less to zero and more of it in the caches, and more words whose slot another word holds)
        constexpr size_t per_slot = 64;
        int bits = 18;
        while (bits < 24 && ((size_t)1 << bits) < (size_t)n_bytes / per_slot) ++bits;
        claim_slots = (size_t)1 << bits;
        w->w_claims.reserve(claim_slots * 16);
        w->w_claim_rows.reserve(claim_slots * 16);
        z.add(w->w_claims.p, claim_slots * 16);
    }
    launch_zero_regions(st, t->n_cu * 4, z);
    out->d_ids = w->w_ids.as<uint32_t>();
    out->d_tok_offsets = w->w_tok_offsets.as<int64_t>();
    out->d_n_tokens = d_ntok_total;
    out->d_n_pretokens = d_npretok;
    out->ids_capacity = ((hm.norm == NORM_NFC && w->device_bound) ? 3 * n_bytes + 64 : n_x) + 4;          // what w_ids holds (a token covers a byte of the X text); the epilogues size theirs from the data
    out->d_offsets = out->d_word_ids = out->d_pad_counts = out->d_enc_docs = out->d_enc_parts = nullptr;
    out->d_type_ids = out->d_seq_ids = nullptr;
    out->d_n_encodings = nullptr;
    w->cur_trim1 = nullptr;
    w->last_n_enc = -1;
    w->last_n_docs = n_docs;
    w->last_seq_off = d_seq_off;
    w->last_n_seqs = n_seqs;
    w->last_inp_off = d_inp_off;
    w->last_n_inputs = n_inputs;
}

void Batch::validate_inputs() {
    // the caller's CSR is validated once; everything below reads the validated copy
    w->w_doc_off.reserve((size_t)(n_docs + 2) * 8);
    // The plain GPT-2 path (no added tokens, no normalizer, no prefix space: BASELINE configs[1] / [4]) reads the document CSR in two
    // places only: the document bitmask, and the documents' first pre-tokens.  The first is built by the validating kernel itself
    // (a bit only from a document that is consistent on its own: always inside the text), the second kernel writes the validated
    // copy on its way (it runs behind the whole validation, so it knows the verdict) -- two launches instead of four
    // (every other tokenizer takes the general order).  A malformed CSR still never turns into an access outside the buffers; the batch
    // fails with TKAMD_ERR_INVALID as before.
    lean = n_bytes > 0 && hm.at[0].size() == 0 && hm.at[1].size() == 0 && (hm.norm == NORM_NONE || (hm.norm == NORM_NFC && !nfc_general)) && !prefix_space &&
           (hm.pretok == PT_BYTELEVEL_GPT2 || hm.pretok == PT_BYTELEVEL_NOREGEX);
    raw_doc_off = d_doc_off;
    if (!lean) {
        pf.begin("validate_csr");
        launch_validate_csr(st, d_doc_off, n_docs, n_bytes, d_err, w->w_doc_off.as<int64_t>());
        pf.end();
    }
    d_doc_off = w->w_doc_off.as<int64_t>();
    if (words_in) {
        w->w_seq_off.reserve((size_t)(n_seqs + 2) * 8);
        w->w_seq_tok_off.reserve((size_t)(n_seqs + 2) * 8);
        launch_validate_csr(st, d_seq_off, n_seqs, n_docs, d_err, w->w_seq_off.as<int64_t>());     // a CSR over [0, n_words]
        d_seq_off = w->w_seq_off.as<int64_t>();
        out->d_tok_offsets = w->w_seq_tok_off.as<int64_t>();
    }
    e_tok_off = words_in ? w->w_seq_tok_off.as<int64_t>() : w->w_tok_offsets.as<int64_t>();
    if (mixed) {
        w->w_inp_off.reserve((size_t)(n_inputs + 2) * 8);
        launch_validate_csr(st, d_inp_off, n_inputs, e_n, d_err, w->w_inp_off.as<int64_t>());      // a CSR over [0, sequences]
        d_inp_off = w->w_inp_off.as<int64_t>();
    }
}

// only empty documents: no tokens, but the post-processor still puts its specials around every one of them
void Batch::empty_batch() {
    HIP_CHECK(hipMemsetAsync(w->w_tok_offsets.p, 0, (size_t)(n_docs + 1) * 8, st));
    if (words_in) HIP_CHECK(hipMemsetAsync(w->w_seq_tok_off.p, 0, (size_t)(n_seqs + 1) * 8, st));
    if (off_mode != TKAMD_OFFSETS_NONE) out->d_offsets = w->w_offsets.as<uint32_t>();
    if (want_words) out->d_word_ids = w->w_word_ids.as<uint32_t>();
}

AddedArgs Batch::args_of(int c) {
    AddedArgs a{t->t_at_blob[c].as<uint8_t>(), t->t_at_off[c].as<uint32_t>(), t->t_at_first[c].as<uint32_t>(), t->t_at_id[c].as<uint32_t>(),
                t->t_at_flags[c].as<uint32_t>(), {0ull, 0ull, 0ull, 0ull}, 0u, {0u, 0u, 0u, 0u}, t->encode_special ? 1u : 0u, (c == 1 && hm.nfc_ws_fold) ? 1u : 0u};
    std::vector<uint32_t> first = hm.at[c].first;
    if (a.ws_fold && first.size() == 257 && first[' ' + 1] > first[' ']) {
        // a pattern that opens with ' ' may start at any \s char: the first bytes of the 25 of them (k_added_candidates)
        std::vector<uint32_t> has(256, 0u);
        for (uint32_t b = 0; b < 256u; ++b) has[b] = first[b + 1] > first[b] ? 1u : 0u;
        for (uint32_t b : {9u, 10u, 11u, 12u, 13u, 0xC2u, 0xE1u, 0xE2u, 0xE3u}) has[b] = 1u;
        for (uint32_t b = 0; b < 256u; ++b) first[b + 1] = first[b] + has[b];       // (only "is the bucket empty" is read below)
    }
    for (uint32_t b = 0; b < 256u && first.size() == 257; ++b)
        if (first[b + 1] > first[b]) {
            a.first_set[b >> 6] |= 1ull << (b & 63);
            if (a.n_first < 4u) a.first_byte[a.n_first] = b;
            ++a.n_first;
        }
    return a;
}

void Batch::scatter_masks(int64_t n_text, const int64_t* len_dev, bool with_end) {
    ull* m4[4] = {w->w_matchmask.as<ull>(), w->w_spanmask.as<ull>(), w->w_stopmask.as<ull>(), w->w_hardmask.as<ull>()};
    // (one launch for the four, and only if an earlier scatter left bits behind)
    ZeroRegions z{};
    // (lazily: the WHOLE buffers -- the bits may be an earlier, larger batch's)
    const size_t cap4[4] = {w->w_matchmask.cap, w->w_spanmask.cap, w->w_stopmask.cap, w->w_hardmask.cap};
    for (int q = 0; q < 4; ++q) z.add(m4[q], cap4[q] & ~(size_t)15);
    z.only_if = w->w_mask_dirty.as<uint32_t>();
    launch_zero_regions(st, t->n_cu * 4, z);
    launch_scatter_matches(st, mlist, n_match, n_text, len_dev, m4[0], m4[1], m4[2], m4[3], with_end ? w->w_tmp_end.as<uint32_t>() : nullptr,
                           w->w_mask_dirty.as<uint32_t>());
}

// pieces of a text: what lies between document edges and match edges (boundary mask = docmask | hardmask), as an int64 CSR
const int64_t* Batch::build_pieces(const int64_t* doc_csr, int64_t n_text, const int64_t* len_dev) {
    const int64_t Wt = (n_text >> 6) + 1;
    HIP_CHECK(hipMemsetAsync(w->w_boundmask.p, 0, WX * 8, st));
    launch_mark_doc_starts_n(st, doc_csr, n_docs, n_text, len_dev, w->w_boundmask.as<ull>(), d_err);
    launch_mask_or(st, w->w_boundmask.as<ull>(), w->w_hardmask.as<ull>(), Wt, n_match);
    w->w_bprefix.reserve((size_t)(Wt + 2) * 4);
    w->w_seg_off.reserve((seg_cap + 2) * 8);
    launch_mask_scan(st, w->w_boundmask.as<ull>(), Wt, w->w_bsum.as<uint32_t>(), w->w_bprefix.as<uint32_t>(), d_nseg);
    launch_emit_boundaries(st, w->w_boundmask.as<ull>(), w->w_bprefix.as<uint32_t>(), n_text, len_dev, d_nseg, w->w_seg_off.as<int64_t>());
    return w->w_seg_off.as<int64_t>();
}

// from here on the X text is the one made on the device
void Batch::read_ntext() {
    x_text = w->w_ntext.as<uint8_t>();
    x_doc_off = w->w_ndoc_off.as<int64_t>();
    x_len_dev = d_xlen;
}

void Batch::normalize_bert() {
    // ---- BertNormalizer: text -> normalised text + original byte range of every normalised byte; the matches of pass 1 are
    // not text (their split carries the raw slice): copied verbatim ----
    w->w_keepmask.reserve(bn_olen_bytes(n_bytes));          // olen + the per-lane totals: output bytes per source byte (kernels.hpp bn_olen_bytes)
    w->w_kprefix.reserve((size_t)(W0 + 1) * 4);             // wsum
    w->w_wbase.reserve((size_t)(W0 + 1) * 4);
    BnTables bt{t->t_bn1.as<uint16_t>(), t->t_bn2.as<uint8_t>(), t->t_bn_map.as<MergeSlot>(), hm.bn_mask, hm.bn_seed,
                hm.bn_clean_text, hm.bn_handle_chinese, hm.bn_strip_accents, hm.bn_lowercase};
    // (a chain of NFD / Lowercase / StripAccents: the same kernels over the chain's own tables, none of the BertNormalizer's steps)
    if (hm.norm == NORM_CHAIN) { bt.clean = bt.cjk = bt.strip = bt.lower = 0u; bt.chain = 1u | (hm.chain_has(CHAIN_LOWERCASE) ? 2u : 0u); }
    const ull* verbatim = nullptr;
    if (have_raw) {
        scatter_masks(n_bytes, nullptr, false);
        launch_mask_or2(st, w->w_boundmask.as<ull>(), w->w_matchmask.as<ull>(), w->w_spanmask.as<ull>(), W0 + 1);
        verbatim = w->w_boundmask.as<ull>();
    }
    pf.begin("bert_normalize");
    launch_bert_normalize(st, bt, d_text, n_bytes, d_doc_off, n_docs, verbatim, w->w_keepmask.as<uint8_t>(), w->w_kprefix.as<uint32_t>(),
                          w->w_bsum.as<uint32_t>(), w->w_wbase.as<uint32_t>(), d_xlen, w->w_ntext.as<uint8_t>(), (uint32_t*)norig, (uint32_t*)norig_e,
                          w->w_ndoc_off.as<int64_t>(), d_err);
    launch_zero_tail(st, w->w_ntext.as<uint8_t>(), d_xlen, TKAMD_TEXT_PAD, w->w_docmask.as<ull>(), W + 1, t->n_cu * 4);
    pf.end();
    if (have_raw) launch_translate_matches_norm(st, mlist, n_match, w->w_keepmask.as<uint8_t>(), w->w_wbase.as<uint32_t>(), n_bytes, d_xlen);
    read_ntext();
}

void Batch::normalize_nfc() {
    // ---- NFC, the general path: text -> normalised text + the source char of every normalised byte (kernels/nfc.hip); the pieces are the
    // documents and what lies between the matches of pass 1, which are copied verbatim ----
    w->w_keepmask.reserve(bn_olen_bytes(n_bytes));
    w->w_kprefix.reserve((size_t)(W0 + 1) * 4);
    w->w_wbase.reserve((size_t)(W0 + 1) * 4);
    w->w_ms_dmask.reserve((size_t)(W0 + 2) * 8);
    HIP_CHECK(hipMemsetAsync(w->w_ms_dmask.p, 0, (size_t)(W0 + 2) * 8, st));
    launch_mark_doc_starts_n(st, d_doc_off, n_docs, n_bytes, nullptr, w->w_ms_dmask.as<ull>(), d_err);
    const ull* verbatim = nullptr;
    if (have_raw) {
        scatter_masks(n_bytes, nullptr, false);
        launch_mask_or2(st, w->w_boundmask.as<ull>(), w->w_matchmask.as<ull>(), w->w_spanmask.as<ull>(), W0 + 1);
        verbatim = w->w_boundmask.as<ull>();
        launch_nfc_bound(st, w->w_ms_dmask.as<ull>(), verbatim, W0 + 1);
    }
    NfcTables nt{t->t_nfc1.as<uint16_t>(), t->t_nfc2.as<uint8_t>(), t->t_nfc_map.as<MergeSlot>(), hm.nfc_mask, hm.nfc_seed};
    if ((nt.mode = hm.nfc_mode()) & NFC_ANY_LOWER) {    // (to_lowercase rides in the BertNormalizer tables' place)
        nt.l1 = t->t_bn1.as<uint16_t>(); nt.l2 = t->t_bn2.as<uint8_t>(); nt.lmap = t->t_bn_map.as<MergeSlot>();
        nt.lmap_mask = hm.bn_mask; nt.lmap_seed = hm.bn_seed;
    }
    pf.begin("nfc_normalize");
    launch_nfc_normalize(st, nt, d_text, n_bytes, d_doc_off, n_docs, verbatim, w->w_ms_dmask.as<ull>(), w->w_keepmask.as<uint8_t>(), w->w_kprefix.as<uint32_t>(),
                         w->w_bsum.as<uint32_t>(), w->w_wbase.as<uint32_t>(), d_xlen, w->w_ntext.as<uint8_t>(), (uint32_t*)norig, w->w_ndoc_off.as<int64_t>(), d_err);
    launch_zero_tail(st, w->w_ntext.as<uint8_t>(), d_xlen, TKAMD_TEXT_PAD, w->w_docmask.as<ull>(), W + 1, t->n_cu * 4);
    pf.end();
    if (have_raw) launch_translate_matches_norm(st, mlist, n_match, w->w_keepmask.as<uint8_t>(), w->w_wbase.as<uint32_t>(), n_bytes, d_xlen);
    read_ntext();
}

void Batch::normalize_precompiled() {
    // ---- Precompiled: text -> normalized text + the source char of every normalized byte (kernels/precompiled.hip); the pieces are the
    // documents and what lies between the matches of pass 1, which are copied verbatim.  The "▁" front reads the result. ----
    const int64_t Wp = (n_p >> 6) + 1;
    w->w_ptext.reserve((size_t)n_p + TKAMD_TEXT_PAD);
    w->w_pdoc_off.reserve((size_t)(n_docs + 2) * 8);
    w->w_pc_ltot.reserve((((size_t)n_bytes >> 4) + 8) * 2);
    w->w_keepmask.reserve(bn_olen_bytes(n_p));              // (sized for the front's pass over the normalized text too: the buffers do not move between the two)
    w->w_kprefix.reserve((size_t)(Wp + 1) * 4);
    w->w_wbase.reserve((size_t)(Wp + 1) * 4);
    w->w_ms_dmask.reserve((size_t)(Wp + 2) * 8);
    if (off_mode != TKAMD_OFFSETS_NONE) w->w_pnorig.reserve(((size_t)n_p + 4) * 4);
    HIP_CHECK(hipMemsetAsync(w->w_ms_dmask.p, 0, (size_t)(W0 + 2) * 8, st));
    launch_mark_doc_starts_n(st, d_doc_off, n_docs, n_bytes, nullptr, w->w_ms_dmask.as<ull>(), d_err);
    const ull* verbatim = nullptr;
    if (have_raw) {
        scatter_masks(n_bytes, nullptr, false);
        launch_mask_or2(st, w->w_boundmask.as<ull>(), w->w_matchmask.as<ull>(), w->w_spanmask.as<ull>(), W0 + 1);
        verbatim = w->w_boundmask.as<ull>();
        launch_nfc_bound(st, w->w_ms_dmask.as<ull>(), verbatim, W0 + 1);
    }
    const PcTables pt{t->t_pc_units.as<uint32_t>(), (uint32_t)hm.pc_units.size(), t->t_pc_rep.as<uint8_t>(), (uint32_t)hm.pc_rep.size(), t->t_gc1.as<uint16_t>(), t->t_gc2.as<uint8_t>(),
                      {hm.pc_first[0], hm.pc_first[1], hm.pc_first[2], hm.pc_first[3]}};
    int64_t* plen = sc + SC_PLEN;
    uint32_t* pnorig = off_mode != TKAMD_OFFSETS_NONE ? w->w_pnorig.as<uint32_t>() : nullptr;
    pf.begin("precompiled_normalize");
    launch_precompiled(st, pt, d_text, n_bytes, d_doc_off, n_docs, verbatim, w->w_ms_dmask.as<ull>(), w->w_keepmask.as<uint8_t>(), w->w_pc_ltot.as<uint16_t>(),
                       w->w_kprefix.as<uint32_t>(), w->w_bsum.as<uint32_t>(), w->w_wbase.as<uint32_t>(), plen, w->w_ptext.as<uint8_t>(), pnorig, w->w_pdoc_off.as<int64_t>(), d_err,
                       t->n_cu * 4, n_p);
    launch_zero_tail(st, w->w_ptext.as<uint8_t>(), plen, TKAMD_TEXT_PAD);
    pf.end();
    if (have_raw) launch_pc_translate_matches(st, mlist, n_match, w->w_keepmask.as<uint8_t>(), w->w_pc_ltot.as<uint16_t>(), w->w_wbase.as<uint32_t>(), n_bytes, plen);
    p_text = w->w_ptext.as<uint8_t>();
    p_doc_off = w->w_pdoc_off.as<int64_t>();
    d_plen = plen;
    p_norig = pnorig;
}

void Batch::normalize_nfkc() {
    // ---- NFKC: text -> normalized text + the source char of every normalized byte (kernels/nfkc.hip, the K mode of the NFC core) in the
    // Precompiled normalizer's arrangement: the pieces are the documents and what lies between the matches of pass 1, which are copied
    // verbatim; pass 2 and the "▁" front read the result. ----
    const int64_t Wp = (n_p >> 6) + 1;
    w->w_ptext.reserve((size_t)n_p + TKAMD_TEXT_PAD);
    w->w_pdoc_off.reserve((size_t)(n_docs + 2) * 8);
    w->w_pc_ltot.reserve((((size_t)n_bytes >> 4) + 8) * 2);
    w->w_keepmask.reserve(bn_olen_bytes(n_p));              // (sized for the front's pass over the normalized text too: the buffers do not move between the two)
    w->w_kprefix.reserve((size_t)(Wp + 1) * 4);
    w->w_wbase.reserve((size_t)(Wp + 1) * 4);
    w->w_ms_dmask.reserve((size_t)(Wp + 2) * 8);
    if (off_mode != TKAMD_OFFSETS_NONE) w->w_pnorig.reserve(((size_t)n_p + 4) * 4);
    HIP_CHECK(hipMemsetAsync(w->w_ms_dmask.p, 0, (size_t)(W0 + 2) * 8, st));
    launch_mark_doc_starts_n(st, d_doc_off, n_docs, n_bytes, nullptr, w->w_ms_dmask.as<ull>(), d_err);
    const ull* verbatim = nullptr;
    if (have_raw) {
        scatter_masks(n_bytes, nullptr, false);
        launch_mask_or2(st, w->w_boundmask.as<ull>(), w->w_matchmask.as<ull>(), w->w_spanmask.as<ull>(), W0 + 1);
        verbatim = w->w_boundmask.as<ull>();
        launch_nfc_bound(st, w->w_ms_dmask.as<ull>(), verbatim, W0 + 1);
    }
    NfcTables nt{t->t_nfc1.as<uint16_t>(), t->t_nfc2.as<uint8_t>(), t->t_nfc_map.as<MergeSlot>(), hm.nfc_mask, hm.nfc_seed};
    nt.lmap = t->t_nfk_map.as<MergeSlot>(); nt.lmap_mask = hm.nfk_mask; nt.lmap_seed = hm.nfk_seed; nt.kflat = t->t_nfk_flat.as<uint32_t>();      // (K mode's slots, nfc_core.hpp)
    int64_t* plen = sc + SC_PLEN;
    uint32_t* pnorig = off_mode != TKAMD_OFFSETS_NONE ? w->w_pnorig.as<uint32_t>() : nullptr;
    pf.begin("nfkc_normalize");
    launch_nfkc_normalize(st, nt, d_text, n_bytes, d_doc_off, n_docs, verbatim, w->w_ms_dmask.as<ull>(), w->w_keepmask.as<uint8_t>(), w->w_pc_ltot.as<uint16_t>(),
                          w->w_kprefix.as<uint32_t>(), w->w_bsum.as<uint32_t>(), w->w_wbase.as<uint32_t>(), plen, w->w_ptext.as<uint8_t>(), pnorig, w->w_pdoc_off.as<int64_t>(), d_err, n_p);
    launch_zero_tail(st, w->w_ptext.as<uint8_t>(), plen, TKAMD_TEXT_PAD);
    pf.end();
    if (have_raw) launch_pc_translate_matches(st, mlist, n_match, w->w_keepmask.as<uint8_t>(), w->w_pc_ltot.as<uint16_t>(), w->w_wbase.as<uint32_t>(), n_bytes, plen);
    p_text = w->w_ptext.as<uint8_t>();
    p_doc_off = w->w_pdoc_off.as<int64_t>();
    d_plen = plen;
    p_norig = pnorig;
    // (pass 2 matches the normalized patterns over this text)
    x_text = p_text;
    x_doc_off = p_doc_off;
    x_len_dev = d_plen;
}

void Batch::shift_behind_prefix_spaces() {
    // ---- ByteLevel add_prefix_space: every piece shifted behind its virtual leading space (byte_level.rs:120-125) ----
    const int64_t* seg = d_doc_off;
    const int64_t* nseg_dev = nullptr;
    int64_t nseg_bound = n_docs;
    if (have_added) {
        scatter_masks(n_bytes, nullptr, false);
        seg = build_pieces(d_doc_off, n_bytes, nullptr);
        nseg_dev = d_nseg;
        nseg_bound = (int64_t)seg_cap;
        w->w_xseg_off.reserve((seg_cap + 2) * 8);
    }
    w->w_need.reserve((size_t)(nseg_bound + 2) * 4);
    w->w_need_bsum.reserve((size_t)((nseg_bound + 1) / 256 + 2) * 4);
    int64_t* xseg = have_added ? w->w_xseg_off.as<int64_t>() : w->w_ndoc_off.as<int64_t>();
    pf.begin("prefix_space");
    launch_prefix_space(st, d_text, seg, nseg_bound, nseg_dev, have_added ? w->w_matchmask.as<ull>() : nullptr, w->w_need.as<uint32_t>(),
                        w->w_need_bsum.as<uint32_t>(), xseg, d_xlen, w->w_ntext.as<uint8_t>(), (uint32_t*)norig, (uint32_t*)norig_e, grid);
    if (have_added) {
        // documents and matches in the shifted text: both start at piece boundaries
        launch_prefix_doc_csr(st, d_doc_off, n_docs, w->w_boundmask.as<ull>(), w->w_bprefix.as<uint32_t>(), n_bytes, nullptr, d_nseg, xseg, w->w_ndoc_off.as<int64_t>());
        launch_translate_matches_prefix(st, mlist, n_match, w->w_boundmask.as<ull>(), w->w_bprefix.as<uint32_t>(), n_bytes, nullptr, d_nseg, xseg);
    }
    pf.end();
    read_ntext();
    if (have_added) {
        scatter_masks(n_x, x_len_dev, off_mode != TKAMD_OFFSETS_NONE);
        matchmask = w->w_matchmask.as<ull>();
        piece_off = xseg;
        piece_n_dev = d_nseg;
    }
}

void Batch::metaspace_front() {
    // ---- the "▁" front: the pieces (documents, and what lies between added-token matches) of the raw text -- behind a Precompiled normalizer:
    // of its output, whose length only the device knows -- -> the "▁" text X + the original byte of every X byte; the matches are copied as
    // they are and move into X coordinates like the normaliser's (kernels/metaspace.hip) ----
    const uint8_t* in_text = precomp ? p_text : d_text;
    const int64_t n_i = precomp ? n_p : n_bytes, Wi = (n_i >> 6) + 1;
    const int64_t* in_len = precomp ? d_plen : nullptr;
    const int64_t* in_doc = precomp ? p_doc_off : d_doc_off;
    w->w_ms_dmask.reserve((size_t)(Wi + 2) * 8);
    HIP_CHECK(hipMemsetAsync(w->w_ms_dmask.p, 0, (size_t)(Wi + 2) * 8, st));
    launch_mark_doc_starts_n(st, in_doc, n_docs, n_i, in_len, w->w_ms_dmask.as<ull>(), d_err);
    const ull* pstart = w->w_ms_dmask.as<ull>();
    if (have_added) {
        scatter_masks(n_i, in_len, false);
        build_pieces(in_doc, n_i, in_len);
        pstart = w->w_boundmask.as<ull>();
    }
    w->w_keepmask.reserve(bn_olen_bytes(n_i));          // output bytes per source byte (kernels.hpp bn_olen_bytes)
    w->w_kprefix.reserve((size_t)(Wi + 1) * 4);
    w->w_wbase.reserve((size_t)(Wi + 1) * 4);
    pf.begin("metaspace");
    launch_metaspace(st, in_text, n_i, in_doc, n_docs, pstart, w->w_ms_dmask.as<ull>(), have_added ? w->w_matchmask.as<ull>() : nullptr,
                     have_added ? w->w_spanmask.as<ull>() : nullptr, (uint32_t)hm.ms_prepend, w->w_keepmask.as<uint8_t>(), w->w_kprefix.as<uint32_t>(),
                     w->w_bsum.as<uint32_t>(), w->w_wbase.as<uint32_t>(), d_xlen, w->w_ntext.as<uint8_t>(), (uint32_t*)norig, w->w_ndoc_off.as<int64_t>(), in_len, p_norig);
    launch_zero_tail(st, w->w_ntext.as<uint8_t>(), d_xlen, TKAMD_TEXT_PAD, w->w_docmask.as<ull>(), W + 1, t->n_cu * 4);
    pf.end();
    if (have_added) launch_translate_matches_norm(st, mlist, n_match, w->w_keepmask.as<uint8_t>(), w->w_wbase.as<uint32_t>(), n_i, d_xlen);
    read_ntext();
    if (have_added) {
        scatter_masks(n_x, x_len_dev, off_mode != TKAMD_OFFSETS_NONE);
        matchmask = w->w_matchmask.as<ull>();
    }
}

void Batch::build_x_text() {
    // ---- AddedVocabulary::extract_and_normalize (added_vocabulary.rs:523-564) + normalizer + ByteLevel add_prefix_space ----
    // Three texts at most: the ORIGINAL one, the X text the pre-tokenizer reads (normalised, or shifted behind prefix spaces), and
    // in between -- with a normalizer -- nothing else: add_prefix_space behind a normalizer is refused above.  Matches are kept as
    // a list (start, stop, id) that is moved from text to text; the bitmasks are scattered from it in the text they are used in.
    const HostModel::PatternSet &setA = hm.at[0], &setB = hm.at[1];
    // Natural text holds no added token: a tokenizer that has some runs the batch as if it had none -- one detection pass per pattern set
    // (k_added_candidates with a note instead of a mask) where match / resolve / scatter / piece launches would find nothing -- and a batch
    // whose text does hold the content of one is run again with the passes below when it is synchronised (NOTE_ADDED_SEEN, finish_batch;
    // the handle's next added_spec_len batches then do not speculate).
    bool spec = (setA.size() > 0 || setB.size() > 0) && t->added_spec_len > 0 && !w->force_general && !(flags & TKAMD_NO_SPECULATION);
    w->force_general = false;
    if (spec) {
        int p = t->added_spec_pause.load();
        while (p > 0 && !t->added_spec_pause.compare_exchange_weak(p, p - 1)) {}
        if (p > 0) spec = false;
    }
    have_raw = setA.size() > 0 && !spec;
    have_norm = setB.size() > 0 && !spec;
    have_added = have_raw || have_norm;
    n_match = d_counters + CNT_MATCHES;
    d_nseg = sc + SC_NSEG;
    WX = (size_t)std::max(W0, W) + 2;             // mask words covering either text
    if (have_added) {
        seg_cap = (size_t)n_docs + 2 * (size_t)mcap + 2;
        DevBuf* masks[6] = {&w->w_candmask, &w->w_matchmask, &w->w_spanmask, &w->w_stopmask, &w->w_hardmask, &w->w_boundmask};
        bool grew = !w->w_mask_dirty.p;
        for (DevBuf* b : masks) { const size_t before = b->cap; b->reserve(WX * 8); grew = grew || b->cap != before; }
        // The four match masks are kept CLEAN between their uses: k_scatter_matches leaves "bits were set" in w_mask_dirty, and the zeroing
        // in front of the next scatter runs only then (natural text holds no special token: 240 MB of zeroing per C3 step went this way).
        // Fresh allocations hold anything: flagged dirty.
        w->w_mask_dirty.reserve(16);
        if (grew) HIP_CHECK(hipMemsetAsync(w->w_mask_dirty.p, 0xFF, 8, st));      // (dirty, as far as the buffers go)
        w->w_match_docs.reserve((seg_cap + 1) * 4);
        w->w_match_list.reserve(((size_t)mcap + 4) * 16);
        mlist = w->w_match_list.as<uint32_t>();
    }
    if (have_added) HIP_CHECK(hipMemsetAsync(n_match, 0, 4, st));
    if (spec && setA.size() > 0) {
        pf.begin("added_token_match");
        launch_added_detect(st, args_of(0), d_text, n_bytes, nullptr, d_err);
        pf.end();
    }
    if (have_raw) {
        // pass 1: the tokens with normalized = false, over the raw documents
        pf.begin("added_token_match");
        launch_added_match(st, args_of(0), d_text, n_bytes, nullptr, d_doc_off, n_docs, nullptr, nullptr, t->dt.uc1, t->dt.uc2, w->w_candmask.as<ull>(),
                           w->w_match_docs.as<uint32_t>(), d_counters + CNT_MATCH_DOCS, mlist, n_match, mcap, MATCH_LEN_ORIG, d_err);
        pf.end();
    }
    x_text = d_text;
    x_doc_off = d_doc_off;
    const bool normalized = hm.norm == NORM_BERT || hm.norm == NORM_CHAIN || nfc_general;      // X is a normaliser's output (the BnOlen layout, norig without ends)
    if (normalized || prefix_space || metaspace) {
        w->w_ntext.reserve((size_t)n_x + TKAMD_TEXT_PAD);
        w->w_ndoc_off.reserve((size_t)(n_docs + 2) * 8);
        // (the prefix-space copy leaves nothing unwritten either, but only the normaliser's path has been taken through the tests without
        // this memset: k_zero_tail behind launch_bert_normalize zeroes the slack behind the text it wrote)
        if (!normalized && !metaspace) HIP_CHECK(hipMemsetAsync(w->w_ntext.p, 0, (size_t)n_x + TKAMD_TEXT_PAD, st));
        // test hook TKAMD_POISON_NTEXT (with TKAMD_TEST_HOOKS=1): the normaliser's output buffer starts every batch as 0xFF, so a kernel that
        // reads it beyond *x_len + TEXT_PAD -- bounded by the host's n_x instead of the device length -- changes a result instead of
        // meeting zeros an earlier batch or the allocator happened to leave (tests/test_parity_gpu.py runs the BertNormalizer fixtures so)
        else if (test_hook("TKAMD_POISON_NTEXT")) {
            HIP_CHECK(hipMemsetAsync(w->w_ntext.p, 0xFF, (size_t)n_x + TKAMD_TEXT_PAD, st));
            // ... and so do the masks and prefix counts over that text: only the words of its own length are written
            // (the document mask's are zeroed behind the normaliser), every reader must stop there too
            HIP_CHECK(hipMemsetAsync(w->w_docmask.p, 0xFF, w->w_docmask.cap, st));
            HIP_CHECK(hipMemsetAsync(w->w_startmask.p, 0xFF, w->w_startmask.cap, st));
            HIP_CHECK(hipMemsetAsync(w->w_wprefix.p, 0xFF, w->w_wprefix.cap, st));
            if (w->w_endmask.p) HIP_CHECK(hipMemsetAsync(w->w_endmask.p, 0xFF, w->w_endmask.cap, st));
        }
        if (off_mode != TKAMD_OFFSETS_NONE) {
            w->w_norig.reserve(((size_t)n_x + 4) * 4);
            norig = w->w_norig.as<uint32_t>();
            // (behind BertNormalizer the END of a byte's original range follows from its start and the original text -- kernels/output.hip
            // norig_end: 4 bytes per normalised byte less to write and to read; the prefix-space copy keeps per-byte ends)
            if (!normalized && !metaspace) {
                w->w_norig_e.reserve(((size_t)n_x + 4) * 4);
                norig_e = w->w_norig_e.as<uint32_t>();
            }
        }
    }
    if (hm.norm == NORM_BERT || (hm.norm == NORM_CHAIN && !hm.nfd_mode())) normalize_bert();
    if (hm.nfd_mode()) normalize_nfc();
    if (hm.norm == NORM_NFC) {
        if (nfc_general) normalize_nfc();
        else {
            pf.begin("nfc_check");
            NfcTables nt{t->t_nfc1.as<uint16_t>(), t->t_nfc2.as<uint8_t>(), t->t_nfc_map.as<MergeSlot>(), hm.nfc_mask, hm.nfc_seed};
            if ((nt.mode = hm.nfc_mode()) & NFC_LOWER) {        // (Lowercase behind NFC: a char that lowercases is one the check does not vouch for)
                nt.l1 = t->t_bn1.as<uint16_t>(); nt.l2 = t->t_bn2.as<uint8_t>(); nt.lmap = t->t_bn_map.as<MergeSlot>();
                nt.lmap_mask = hm.bn_mask; nt.lmap_seed = hm.bn_seed;
            }
            launch_nfc_check(st, nt, d_text, n_bytes, d_err);
            pf.end();
        }
    }
    if (nfkc) normalize_nfkc();
    else if (precomp) normalize_precompiled();
    n_in = normalized ? n_x : nfkc ? n_p : n_bytes;
    if (spec && setB.size() > 0) {
        pf.begin("added_token_match2");
        launch_added_detect(st, args_of(1), x_text, n_in, x_len_dev, d_err);
        pf.end();
    }
    if (have_norm) {
        // pass 2: the tokens with normalized = true, by their normalised patterns, over every piece pass 1 left (the whole documents
        // when it found nothing or there is no such token)
        const int64_t* seg = x_doc_off;
        const int64_t* nseg_dev = nullptr;
        int64_t nseg_bound = n_docs;
        if (have_raw) {
            scatter_masks(n_in, x_len_dev, false);
            seg = build_pieces(x_doc_off, n_in, x_len_dev);
            nseg_dev = d_nseg;
            nseg_bound = (int64_t)seg_cap;
        }
        pf.begin("added_token_match2");
        launch_added_match(st, args_of(1), x_text, n_in, x_len_dev, seg, nseg_bound, nseg_dev, have_raw ? w->w_matchmask.as<ull>() : nullptr, t->dt.uc1, t->dt.uc2,
                           w->w_candmask.as<ull>(), w->w_match_docs.as<uint32_t>(), d_counters + CNT_MATCH_DOCS2, mlist, n_match, mcap,
                           (normalized || nfkc) ? 0u : MATCH_LEN_ORIG, d_err);
        pf.end();
    }
    if (have_added && !prefix_space && !metaspace) {
        scatter_masks(n_in, x_len_dev, off_mode != TKAMD_OFFSETS_NONE);
        matchmask = w->w_matchmask.as<ull>();
    }
    // (piece_off: sentence CSR for the Llama-3 sequential matcher when matches cut the documents)
    if (prefix_space) shift_behind_prefix_spaces();
    else if (metaspace) metaspace_front();
    else if (have_added && (hm.pretok == PT_LLAMA3 || hm.pretok == PT_SPLIT_CHAIN)) {
        piece_off = build_pieces(x_doc_off, n_in, x_len_dev);
        piece_n_dev = d_nseg;
    }
}

void Batch::pretokenize() {
    pf.begin("mark_doc_starts");
    launch_mark_doc_starts_n(st, lean ? raw_doc_off : x_doc_off, n_docs, n_x, x_len_dev, w->w_docmask.as<ull>(), d_err);
    if (matchmask) launch_mask_or(st, w->w_docmask.as<ull>(), w->w_hardmask.as<ull>(), W, n_match);   // match edges are hard boundaries
    pf.end();
    // char offsets over a text the pre-tokenizer reads as it came: the lead-byte mask rides along in its lane kernel (where that has the form)
    const bool text_as_it_came = off_mode == TKAMD_OFFSETS_CHAR && x_text == d_text && !x_len_dev && n_x == n_bytes;
    const auto ride_lead = [&] {
        w->w_leadmask.reserve((size_t)(W0 + 1) * 8);
        lead_done = true;
    };
    if (hm.pretok == PT_BYTELEVEL_GPT2) {
        pf.begin("pretok_gpt2_seq");
        if (text_as_it_came) ride_lead();
        launch_pretok_gpt2(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2, w->w_startmask.as<ull>(), lead_done ? w->w_leadmask.as<ull>() : nullptr);
        pf.end();
    } else if (hm.pretok == PT_LLAMA3) {
        w->w_endmask.reserve((size_t)(W + 1) * 8);          // reused as the "unresolved" mask
        w->w_slow_docs.reserve((size_t)(n_docs + 1) * 4);
        // (the lane kernel of the bit-parallel members)
        if (text_as_it_came && (split_rule_fast(hm.split_rule) || (split_rule_fast_cs(hm.split_rule) && t->t_ucc1.p))) ride_lead();
        pf.begin("pretok_llama3");
        w->w_slow_docs.reserve((size_t)((piece_off ? seg_cap : (size_t)n_docs) + 1) * 4);
        launch_pretok_llama3(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2, w->w_startmask.as<ull>(),
                             w->w_endmask.as<ull>(), piece_off ? piece_off : x_doc_off, piece_off ? (int64_t)seg_cap : n_docs, piece_n_dev,
                             w->w_slow_docs.as<uint32_t>(), d_counters + CNT_SLOW_DOCS, hm.split_rule,
                             t->t_ucc1.p ? t->t_ucc1.as<uint16_t>() : nullptr, t->t_ucc2.p ? t->t_ucc2.as<uint8_t>() : nullptr,
                             w->w_l3_tiles.p ? w->w_l3_tiles.as<ull>() : nullptr, lead_done ? w->w_leadmask.as<ull>() : nullptr);
        pf.end();
    } else if (hm.pretok == PT_SPLIT_CHAIN) {
        // the chained Split of DeepSeek-V3 / R1: the lane kernel, then the sequential matcher on the sentences it left a byte of undecided
        w->w_endmask.reserve((size_t)(W + 1) * 8);          // reused as the "unresolved" mask
        if (text_as_it_came) ride_lead();
        pf.begin("pretok_ds3");
        w->w_slow_docs.reserve((size_t)((piece_off ? seg_cap : (size_t)n_docs) + 1) * 4);
        launch_pretok_ds3(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2, t->t_ucc1.as<uint16_t>(), t->t_ucc2.as<uint8_t>(),
                          w->w_startmask.as<ull>(), w->w_endmask.as<ull>(), piece_off ? piece_off : x_doc_off, piece_off ? (int64_t)seg_cap : n_docs, piece_n_dev,
                          w->w_slow_docs.as<uint32_t>(), d_counters + CNT_SLOW_DOCS, lead_done ? w->w_leadmask.as<ull>() : nullptr);
        pf.end();
    } else if (hm.pretok == PT_DIGITS_GPT2) {
        // Sequence[Digits, ByteLevel] of the StarCoder family: the GPT-2 rule inside the pieces Digits cuts, one lane kernel
        if (text_as_it_came) ride_lead();
        pf.begin("pretok_digits");
        launch_pretok_digits(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2, hm.digits_individual, w->w_startmask.as<ull>(),
                             lead_done ? w->w_leadmask.as<ull>() : nullptr);
        pf.end();
    } else if (hm.pretok == PT_BLOOM) {
        // Split(BLOOM's pattern, Isolated) + ByteLevel(use_regex=false): the pieces the Split leaves are the pre-tokens, one lane kernel
        if (text_as_it_came) ride_lead();
        pf.begin("pretok_bloom");
        launch_pretok_bloom(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2, w->w_startmask.as<ull>(), lead_done ? w->w_leadmask.as<ull>() : nullptr);
        pf.end();
    } else if (hm.pretok == PT_CLIP) {
        // Split(the CLIP pattern, Removed, inverted) + ByteLevel: one lane kernel writes the starts and the ends -- the \s runs belong to no
        // pre-token -- and the lookup, the merges' queues and the offsets take the ends from the mask, as behind the word models' pre-tokenizers
        w->w_endmask.reserve((size_t)(W + 1) * 8);
        has_end = true;
        if (text_as_it_came) ride_lead();
        pf.begin("pretok_clip");
        launch_pretok_clip(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2, w->w_startmask.as<ull>(), w->w_endmask.as<ull>(),
                           lead_done ? w->w_leadmask.as<ull>() : nullptr);
        pf.end();
    } else if (metaspace) {
        // every piece start (the document mask holds the match edges now) and every "▁" behind another char (or every "▁": split)
        pf.begin("metaspace_units");
        launch_ms_units(st, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), w->w_startmask.as<ull>(), W, hm.ms_split);
        pf.end();
    } else if (hm.pretok == PT_BYTELEVEL_NOREGEX) {
        // ByteLevel(use_regex=false): every document is one pre-token (byte_level.rs:128-130)
        HIP_CHECK(hipMemcpyAsync(w->w_startmask.p, w->w_docmask.p, (size_t)W * 8, hipMemcpyDeviceToDevice, st));
    } else {
        w->w_endmask.reserve((size_t)(W + 1) * 8);
        has_end = true;
        if (want_meta) {
            w->w_pt_end.reserve(((size_t)n_x + 4) * 4);
            pt_end = w->w_pt_end.as<uint32_t>();
        }
        pf.begin("pretok_local");
        launch_pretok_local(st, (int)hm.pretok, x_text, n_x, x_len_dev, w->w_docmask.as<ull>(), t->dt.uc1, t->dt.uc2,
                            w->w_startmask.as<ull>(), w->w_endmask.as<ull>(), true);
        pf.end();
    }
    if (matchmask)
        launch_apply_matches(st, w->w_startmask.as<ull>(), has_end ? w->w_endmask.as<ull>() : nullptr, matchmask, w->w_spanmask.as<ull>(),
                             w->w_stopmask.as<ull>(), W, n_match);
    pf.begin("mask_scan");
    // (three launches: reduce, a one-workgroup scan of the totals, down.  A single-pass ticket + look-back kernel in their place measured
    // 0.031 ms against 0.015: 917 tickets on one address and a look-back chain cost more than two launch gaps, profiles/r4a_*)
    meta_masks = want_meta && !(hm.char_bpe && !hm.unk_configured && !hm.byte_fallback);       // (that one: k_token_meta_seq, from pt_start / pt_end)
    if (meta_masks) w->w_tile_w.reserve(((size_t)n_x / META_TILE + 4) * 4);
    launch_mask_scan(st, w->w_startmask.as<ull>(), W, w->w_bsum.as<uint32_t>(), w->w_wprefix.as<uint32_t>(), d_npretok, x_len_dev,
                     meta_masks ? w->w_tile_w.as<uint32_t>() : nullptr);
    pf.end();
    if (want_meta && !meta_masks) {
        // the pre-token offsets themselves are only materialised for the offsets / word-id pass of the pre-tokenizers WITH an end mask
        // (and of BPE over characters without an unk_token: k_token_meta_seq); the others' k_token_meta reads the start mask itself
        pf.begin("emit_pretok");
        launch_emit_pretok(st, w->w_startmask.as<ull>(), w->w_wprefix.as<uint32_t>(), n_x, x_len_dev, d_npretok, w->w_pt_start.as<uint32_t>());
        if (pt_end) launch_emit_pretok_end(st, w->w_startmask.as<ull>(), w->w_endmask.as<ull>(), w->w_wprefix.as<uint32_t>(), n_x, x_len_dev, pt_end);
        pf.end();
    }
    pf.begin("doc_first_pretok");
    launch_doc_first_pretok(st, lean ? raw_doc_off : x_doc_off, n_docs, n_x, w->w_startmask.as<ull>(), w->w_wprefix.as<uint32_t>(),
                            d_npretok, w->w_doc_pt.as<uint32_t>(), w->w_chunk_lo.as<uint32_t>(),
                            lean ? d_err : nullptr, lean ? w->w_doc_off.as<int64_t>() : nullptr);
    pf.end();
    // the "▁" front over whole pieces: a word id is the index of the pre-token's PIECE in its document, not of the unit (the piece starts are
    // the document mask's bits by now: documents + match edges)
    if (metaspace && !hm.ms_split && want_words && !words_in) {
        w->w_pprefix.reserve((size_t)(W + 2) * 4);
        w->w_pt_word.reserve(((size_t)n_x + 4) * 4);
        pf.begin("metaspace_words");
        launch_mask_scan(st, w->w_docmask.as<ull>(), W, w->w_bsum.as<uint32_t>(), w->w_pprefix.as<uint32_t>(), sc + SC_NPIECE, x_len_dev);
        launch_ms_piece_rank(st, w->w_startmask.as<ull>(), w->w_wprefix.as<uint32_t>(), w->w_docmask.as<ull>(), w->w_pprefix.as<uint32_t>(), n_x, x_len_dev,
                             w->w_pt_word.as<uint32_t>());
        pf.end();
        pt_word = w->w_pt_word.as<uint32_t>();
    }
}

// test hook TKAMD_PHASES: the lookup and the compaction run as their diagnostic instantiations, which add the shader-clock
// ticks of their phases to a table of this workspace (tkamd_debug_phases reads and clears it); never in a measured run
void* Batch::phases_of(int which) {
    if (!test_hook("TKAMD_PHASES")) return nullptr;
    if (!w->w_phases.p) {
        w->w_phases.reserve(2 * PHASE_WGS * 64);
        HIP_CHECK(hipMemsetAsync(w->w_phases.p, 0, 2 * PHASE_WGS * 64, st));
    }
    return (uint8_t*)w->w_phases.p + (size_t)which * PHASE_WGS * 64;
}

// (claims: see zero_batch_state; with offsets k_token_meta takes the token ends of a shared row from the claimant's slots of tmp_end)
void Batch::open_word_cache() {
    const size_t slots = (size_t)1 << WORD_CACHE_BITS;
    if (use_claims) {
        uint32_t* cpos = nullptr;                        // (the claimants' first bytes: only k_token_meta wants them)
        if (off_mode != TKAMD_OFFSETS_NONE) { w->w_claim_pos.reserve(claim_slots * 4); cpos = w->w_claim_pos.as<uint32_t>(); }
        wc = WordCache{nullptr, w->w_claim_rows.p, (unsigned long long*)w->w_claims.p, (uint32_t)(claim_slots - 1), cpos};
        return;
    }
    if (!t->word_cache || off_mode != TKAMD_OFFSETS_NONE) return;        // (a cached row carries no token ends)
    w->w_cache_keys.reserve(slots * sizeof(CacheKey));
    w->w_cache_rows.reserve(slots * 16);
    const uint64_t epoch = t->cache_epoch;
    if (w->cache_epoch != epoch) {
        HIP_CHECK(hipMemsetAsync(w->w_cache_keys.p, 0, slots * sizeof(CacheKey), st));
        w->cache_epoch = epoch;
    }
    wc = WordCache{(CacheKey*)w->w_cache_keys.p, w->w_cache_rows.p, nullptr, 0u, nullptr};
}

// The census behind the hot table (tkamd_tokenizer::hot_adapt): on the handle's first batch of hot_min_bytes of text or more (the caller's bytes: n_x is a host-side BOUND, three
// times the text behind a normalizer) and on every
// hot_period-th such batch after it, on the batch's own stream in front of its lookup.  lt: the tables as this batch's lookup reads them
// (ignore_merges says whether every hit is final).  The synchronisation of the batch reads the counts (read_scalars).
void Batch::hot_census(const DevTables& lt, const ull* endmask) {
    if (!t->hot_adapt || !t->hot_adapt_allowed || n_bytes < t->hot_min_bytes || t->hot_of_slot.empty()) return;
    if (t->hot_gen.load() + 1 >= HOT_RING) return;             // (every buffer of the ring is in use: the handle keeps the table it has)
    if (t->hot_eligible.fetch_add(1) % (uint64_t)t->hot_period) return;
    const size_t words = t->hot_of_slot.size() + 1;
    w->w_hot_hist.reserve(words * 4);
    HIP_CHECK(hipMemsetAsync(w->w_hot_hist.p, 0, words * 4, st));
    pf.begin("hot_census");
    launch_hot_census(st, lt, x_text, n_x, x_len_dev, w->w_startmask.as<ull>(), endmask, matchmask, w->w_hot_hist.as<uint32_t>());
    pf.end();
    w->census_pending = true;
}

void Batch::run_model() {
    tmp_end = (off_mode != TKAMD_OFFSETS_NONE) ? w->w_tmp_end.as<uint32_t>() : nullptr;
    const size_t N = (size_t)n_x;
    const QueueSizes qz = queue_sizes(N, t->q16_div, lookup_grid(t));
    // (TKAMD_ROW_LIMIT_BITS: a test lowers the threshold -- never the 30 bits tok0 really has -- to see the refusal without a 3 GB batch)
    static const size_t row_limit = [] { const char* e = test_hook("TKAMD_ROW_LIMIT_BITS"); return e ? std::min<size_t>((size_t)1 << std::max(8, atoi(e)), ROW_INDEX_LIMIT) : (size_t)ROW_INDEX_LIMIT; }();
    if (qz.total >= row_limit) throw Invalid("batch too large for the work queues (row indices are 30-bit: about 3 GB of text): split it");
    QueuePlan plan{};
    for (int c = 0; c < 4; ++c) {
        plan.v[c].q = (QItem*)(w->w_queues.as<uint8_t>() + (size_t)qz.row_base[c] * 8);
        plan.v[c].counts = w->w_qcount.as<uint32_t>() + (size_t)c * NSQ * QCNT_STRIDE;
        plan.v[c].sq_cap = qz.sq_cap[c];
        plan.v[c].row_base = qz.row_base[c];
    }
    const ull* endmask = has_end ? w->w_endmask.as<ull>() : nullptr;
    // the model kernels end an entry by publishing its row if it holds a claim (bpe.hip claim_publish_item)
    DevTables mdt = t->dt;
    mdt.err = d_err;
    mdt.probes = t->prof ? d_counters + CNT_MERGE_PROBES : nullptr;
    auto set_publish = [&]() {
        if (wc.claims) { mdt.pub_rows = wc.rows; mdt.pub_mask = wc.claim_mask; mdt.pub_pos = wc.claim_pos; }
    };
    if (hm.model == MODEL_BPE) {
        hot_census(t->dt, endmask);
        pf.begin("lookup");
        open_word_cache();
        set_publish();
        launch_lookup(st, lookup_grid(t), t->dt, x_text, n_x, x_len_dev, w->w_startmask.as<ull>(), endmask, w->w_wprefix.as<uint32_t>(),
                      w->w_tok0.as<uint32_t>(), plan, d_err, matchmask, t->hot_cur.load(), wc, 0u, 0u, phases_of(0), d_counters);
        pf.end();
        if (hm.ignore_merges)                              // vocab.get(sequence) for pre-tokens beyond the 16-byte keys (bpe/model.rs:559-567)
            launch_long_vocab3(st, t->n_cu, t->dt, x_text, plan.v[1], plan.v[2], plan.v[3], w->w_rows.p, 0u, d_err, wc);
        // the LDS kernels need new_id = rank + c (true of every trainer-made vocabulary); otherwise -- and under the test hook
        // TKAMD_FORCE_LANE_MERGE -- the register-resident lane kernels run
        const bool lds = t->dt.newid_affine && !test_hook("TKAMD_FORCE_LANE_MERGE");      // keys in LDS
        // With the claims on both queues hold the distinct words only, and a launch of the LDS kernels lasts as long as its longest word's
        // chain of dependent merge probes whatever it holds: ONE launch takes both queues, the 16-symbol and the 32-symbol body side by
        // side in one grid (k_bpe_merge_lds_pair: it splits its workgroups between the queues by their fills, thin or fat, on the device).
        // (Test hooks.  TKAMD_MERGE_TWO: two launches, each kernel with its own queue.  TKAMD_MERGE_PAIR=0: the one launch is the 32-symbol
        // kernel with the <= 16-byte queue behind its own, what ran before the pair kernel -- the A/B of the two in one process.)
        const bool can_one = wc.claims && lds && !test_hook("TKAMD_MERGE_TWO");
        const char* const pair_hook = test_hook("TKAMD_MERGE_PAIR");
        const bool pair = can_one && !(pair_hook && pair_hook[0] == '0');
        const bool one = can_one && !pair;
        w->last_pair_grid = 0u;
        // BPE over characters: only the kernels that know its start (kernels/bpe.hip CHARS) -- the two LDS kernels, each on its own queue,
        // and the workgroup-per-pre-token kernel for everything beyond 32 bytes (or for everything, when the vocabulary's new ids are not
        // in merge order and the LDS kernels cannot run)
        // pre-tokens beyond the LDS path (> 8192 B) run from a global scratch slab: 5 words per symbol, sized for the worst case this batch
        // can contain (the whole X text being such pre-tokens), capped at 1 GiB
        const size_t huge_words = std::min<size_t>((size_t)6 * N + 4096, (size_t)1 << 28);
        const bool huge_possible = N > (size_t)LONG_PT_MAX;
        if (huge_possible) {
            w->w_huge.reserve(huge_words * 4);
            w->w_list_huge.reserve((N / LONG_PT_MAX + 16) * 4);
        } else {
            w->w_huge.reserve(64);
            w->w_list_huge.reserve(64);
        }
        // the longest queue; its pre-tokens beyond 8 KB -- a CJK paragraph is one unit behind the "▁" front -- go on to k_bpe_merge_huge
        auto long_tail = [&]() {
            launch_bpe_merge_long(st, t->n_cu, mdt, x_text, plan.v[3], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end, w->w_list_huge.as<uint32_t>(),
                                  d_counters + CNT_LISTH, w->w_huge.as<uint32_t>(), (unsigned long long)(huge_possible ? huge_words : 0),
                                  (unsigned long long*)(sc + SC_HUGE_USED), d_err);
        };
        if (hm.char_bpe) {
            auto long_only = [&](const QView& q) {
                launch_bpe_merge_long_only(st, t->n_cu * 2, mdt, x_text, q, w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end, w->w_list_huge.as<uint32_t>(), d_counters + CNT_LISTH);
            };
            pf.begin("bpe_merge_lds32");
            if (t->dt.newid_affine) launch_bpe_merge(st, t->n_cu, 6, mdt, x_text, plan.v[1], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end, nullptr);
            else long_only(plan.v[1]);
            pf.end();
            pf.begin("bpe_merge_lds");
            if (t->dt.newid_affine) launch_bpe_merge(st, t->n_cu, 5, mdt, x_text, plan.v[0], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end);
            else long_only(plan.v[0]);
            pf.end();
            pf.begin("bpe_merge_long");
            long_only(plan.v[2]);
            long_tail();
            pf.end();
        } else {
            if (pair) {
                pf.begin("bpe_merge_lds_pair");
                w->last_pair_grid = (uint32_t)launch_bpe_merge_pair(st, t->n_cu, t->pair_grid, mdt, x_text, plan.v[0], plan.v[1], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end);
                pf.end();
            } else {
                pf.begin(lds ? "bpe_merge_lds32" : "bpe_merge_lane32");
                launch_bpe_merge(st, lds ? t->n_cu : grid, lds ? 6 : 2, mdt, x_text, plan.v[1], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end, one ? &plan.v[0] : nullptr);
                pf.end();
            }
            if (!can_one) {
                pf.begin(lds ? "bpe_merge_lds" : "bpe_merge_lane");
                launch_bpe_merge(st, lds ? t->n_cu : grid, lds ? 5 : 1, mdt, x_text, plan.v[0], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end);
                pf.end();
            }
            pf.begin("bpe_merge64");
            launch_bpe_merge(st, grid, 64, mdt, x_text, plan.v[2], w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end);
            pf.end();
            pf.begin("bpe_merge_long");
            long_tail();
            pf.end();
        }
        if (wc.keys) {
            pf.begin("word_cache_insert");
            launch_word_cache_insert(st, grid, mdt, x_text, plan.v[0], w->w_rows.p, wc);
            pf.end();
        }
    } else if (hm.model == MODEL_UNIGRAM) {
        // Unigram::tokenize (unigram/model.rs:443-477): the lookup settles a pre-token that is a piece whose own Viterbi was proved at load
        // to yield [id] (WORD_DIRECT; no other hit is final), the claims keep one occurrence of every other word, and the Unigram kernel
        // runs the search on those.  (The reference's per-model cache changes no result; the word cache across batches stays closed.)
        if (use_claims) open_word_cache();
        set_publish();
        hot_census(t->dt, endmask);
        pf.begin("lookup");
        launch_lookup(st, lookup_grid(t), t->dt, x_text, n_x, x_len_dev, w->w_startmask.as<ull>(), endmask, w->w_wprefix.as<uint32_t>(),
                      w->w_tok0.as<uint32_t>(), plan, d_err, matchmask, t->hot_cur.load(), wc, 0u, 0u, phases_of(0), d_counters);
        pf.end();
        w->w_uni_state.reserve(N > 64 ? (N + 2) * 16 : 64);      // (a word beyond 64 bytes keeps its state at its own bytes: kernels/unigram.hip)
        pf.begin("unigram");
        launch_unigram_all(st, grid, t->n_cu, mdt, x_text, plan, w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end, d_err, w->w_uni_state.p);
        pf.end();
    } else if (hm.model == MODEL_WORDLEVEL) {
        // WordLevel::tokenize (wordlevel/mod.rs:162-178) is the lookup itself: every hit is final, a miss is the unk id
        DevTables wt = t->dt;
        wt.ignore_merges = 1;
        hot_census(wt, endmask);
        pf.begin("wordlevel_lookup");
        launch_lookup(st, lookup_grid(t), wt, x_text, n_x, x_len_dev, w->w_startmask.as<ull>(), endmask, w->w_wprefix.as<uint32_t>(),
                      w->w_tok0.as<uint32_t>(), plan, d_err, matchmask, t->hot_cur.load(), WordCache{nullptr, nullptr, nullptr, 0u, nullptr}, 0u, 1u, nullptr, nullptr);
        launch_long_vocab3(st, t->n_cu, wt, x_text, plan.v[1], plan.v[2], plan.v[3], w->w_rows.p, 1u, d_err, WordCache{nullptr, nullptr, nullptr, 0u, nullptr});      // words longer than 16 bytes
        pf.end();
    } else {
        // WordPiece's first candidate is the whole word (wordpiece/mod.rs:245-258 starts at end = len): the whole-word lookup
        // settles most words with one probe; only the rest walk the trie.  With max_input_chars_per_word < 16 a whole-word
        // hit could belong to a word over the limit, so every word takes the walk (which counts the chars).
        const bool shortcut = hm.max_input_chars >= (uint32_t)WORD_MAX_KEY;
        DevTables wt = t->dt;
        wt.ignore_merges = 1;                              // any whole-word hit is final
        wt.long_probe_max_len = hm.max_input_chars;        // len <= limit  =>  chars <= limit
        // (the reference keeps no cache for WordPiece; a word's pieces depend on nothing but the word, so the same table serves. With
        // every word taking the walk -- max_input_chars_per_word < 16 -- the lookup probes nothing, the cache included.)
        if (shortcut) open_word_cache();
        set_publish();
        if (shortcut) hot_census(wt, endmask);                 // (without the shortcut the lookup probes no table)
        pf.begin("wordpiece_word_lookup");
        launch_lookup(st, lookup_grid(t), wt, x_text, n_x, x_len_dev, w->w_startmask.as<ull>(), endmask, w->w_wprefix.as<uint32_t>(),
                      w->w_tok0.as<uint32_t>(), plan, d_err, matchmask, t->hot_cur.load(), wc, shortcut ? 0u : 1u, 0u, phases_of(0), d_counters);
        pf.end();
        pf.begin("wordpiece");
        launch_wordpiece_all(st, grid, t->n_cu, mdt, x_text, plan, w->w_rows.p, w->w_tmp_ids.as<uint32_t>(), tmp_end, d_err);      // the <= 16-byte queue and the words longer than that, side by side
        pf.end();
        if (wc.keys) {
            pf.begin("word_cache_insert");
            launch_word_cache_insert(st, grid, t->dt, x_text, plan.v[0], w->w_rows.p, wc);
            pf.end();
        }
    }
    if (matchmask)
        launch_apply_match_ids(st, w->w_match_list.as<uint32_t>(), d_counters + CNT_MATCHES, w->w_startmask.as<ull>(),
                               w->w_wprefix.as<uint32_t>(), w->w_tok0.as<uint32_t>());
}

void Batch::compact_and_meta() {
    // with offsets: one byte per token next to the ids -- the boundary in front of the token, where its row carried it (results.hip)
    uint8_t* tok_b8 = nullptr;
    if (tmp_end) { w->w_tok_b8.reserve((size_t)n_x + 64); tok_b8 = w->w_tok_b8.as<uint8_t>(); }
    pf.begin("compact");
    // (the token offsets of the pre-tokens are only materialised for the offsets / word-id pass; the documents' token CSR comes out of the compaction itself)
    launch_compact(st, t->cp_grid, w->w_tok0.as<uint32_t>(), w->w_rows.p, wc.rows, w->w_tmp_ids.as<uint32_t>(), d_npretok, w->w_cstate.as<ull>(),
                   d_ntok_total, want_meta ? w->w_pt_tokoff.as<uint32_t>() : nullptr, w->w_ids.as<uint32_t>(), w->w_chunk_lo.as<uint32_t>(),
                   w->w_doc_pt.as<uint32_t>(), n_docs, w->w_tok_offsets.as<int64_t>(), (size_t)t->cp_grid <= PHASE_WGS ? phases_of(1) : nullptr, tok_b8);
    pf.end();
    const uint32_t* word_of_doc = nullptr;
    const int64_t* first_tok = nullptr;
    if (words_in) {
        // the words' token CSR -> the sequences'; the word id of a token is its word's index in the sequence
        if (want_words) { w->w_word_idx.reserve((size_t)(n_docs + 2) * 4); word_of_doc = w->w_word_idx.as<uint32_t>(); }
        if (off_mode != TKAMD_OFFSETS_NONE && hm.trim_offsets) { w->w_first_tok.reserve((size_t)(n_docs + 2) * 8); first_tok = w->w_first_tok.as<int64_t>(); }
        launch_seq_regroup(st, d_seq_off, n_seqs, n_docs, w->w_tok_offsets.as<int64_t>(), w->w_seq_tok_off.as<int64_t>(), (uint32_t*)word_of_doc, (int64_t*)first_tok);
    }
    if (want_meta) {
        MetaArgs a{};
        a.word_of_doc = word_of_doc;
        a.pt_word = pt_word;
        a.first_tok = first_tok;
        a.x_text = x_text;
        a.text = d_text;
        a.pt_start = meta_masks ? nullptr : w->w_pt_start.as<uint32_t>();
        a.pt_end = meta_masks ? nullptr : pt_end;
        a.startmask = w->w_startmask.as<ull>();
        a.endmask = has_end ? w->w_endmask.as<ull>() : nullptr;
        a.wprefix = w->w_wprefix.as<uint32_t>();
        a.tile_w = meta_masks ? w->w_tile_w.as<uint32_t>() : nullptr;
        a.n_mask_words = W;
        a.x_len_dev = x_len_dev;
        a.x_len_host = n_x;
        a.n_tok = d_ntok_total;
        a.pt_tokoff = w->w_pt_tokoff.as<uint32_t>();
        a.tmp_end = tmp_end;
        a.tok_b8 = tok_b8;
        a.tok0 = wc.claims ? w->w_tok0.as<uint32_t>() : nullptr;
        a.claim_pos = wc.claims ? wc.claim_pos : nullptr;
        a.n_pretok = d_npretok;
        a.doc_pt = w->w_doc_pt.as<uint32_t>();
        a.chunk_lo = w->w_chunk_lo.as<uint32_t>();
        a.chunk = (uint32_t)COMPACT_CHUNK;
        a.n_docs = n_docs;
        a.x_doc_off = x_doc_off;
        a.doc_off = d_doc_off;
        a.norig = norig;                                   // normalised / shifted text: every byte's original byte range
        a.norig_e = norig_e;
        a.byte_level = hm.byte_level;
        a.snap_chars = hm.byte_level || hm.char_bpe || hm.uni_bytes;      // (Unigram's <0xXX> tokens cut their char like BPE's)
        if (hm.char_bpe && !hm.unk_configured && !hm.byte_fallback) {      // (chars can be dropped: offsets are running sums)
            a.char_id = t->dt.char_id;
            a.cb = t->dt.cb;
            if (hm.ignore_merges) { a.ww_tok0 = w->w_tok0.as<uint32_t>(); a.ww_rows = w->w_rows.p; a.ww_crows = wc.rows; }      // (... but not on a whole-word hit)
        }
        a.trim_offsets = hm.trim_offsets;
        a.trim_matches_only = !hm.byte_level;            // (a model that is not byte-level: only an added token's slice can hold what is trimmed; the loader checked the vocabulary)
        a.trim_token_text = hm.model == MODEL_UNIGRAM && !hm.uni_bytes;
        a.pp_add_prefix_space = hm.pp_add_prefix_space;
        a.want_offsets = off_mode != TKAMD_OFFSETS_NONE;
        a.char_mode = off_mode == TKAMD_OFFSETS_CHAR;
        a.want_words = want_words;
        a.matchmask = matchmask;
        a.uc1 = t->dt.uc1;
        a.uc2 = t->dt.uc2;
        a.offsets = w->w_offsets.as<uint32_t>();
        a.word_ids = w->w_word_ids.as<uint32_t>();
        if (a.want_offsets && a.trim_offsets && a.pp_add_prefix_space && hm.trunc_on) {      // (see MetaArgs::trim1)
            w->w_trim1.reserve((size_t)n_x + 8);
            a.trim1 = w->w_trim1.as<uint8_t>();
            w->cur_trim1 = a.trim1;
        }
        if (a.char_mode) {
            w->w_leadmask.reserve((size_t)(W0 + 1) * 8);
            w->w_lprefix.reserve((size_t)(W0 + 1) * 4);
            pf.begin("leadmask_scan");
            if (!lead_done) launch_leadmask(st, d_text, n_bytes, w->w_leadmask.as<ull>());
            launch_mask_scan(st, w->w_leadmask.as<ull>(), W0, w->w_bsum.as<uint32_t>(), w->w_lprefix.as<uint32_t>(), sc + SC_NCHARS);
            pf.end();
            a.leadmask = w->w_leadmask.as<ull>();
            a.lprefix = w->w_lprefix.as<uint32_t>();
        }
        pf.begin("token_meta");
        launch_token_meta(st, grid, a);
        pf.end();
        if (a.want_offsets && hm.uni_bytes) {
            // Unigram byte_fallback: every <0xXX> token of a run carries the WHOLE run's offsets (unigram/model.rs:459); token_meta gave each
            // its own char's.  The documents' token CSR (the words', for pre-tokenized input): a run never crosses a document.
            // k_unigram_run_offsets reads the runs off the result; what it relies on: (1) split = true, so every pre-token that follows another
            // inside a piece begins with a U+2581 (k_ms_units marks every U+2581; refused otherwise, host_model.cpp); (2) that U+2581 is a piece
            // and the unk piece does not begin with one, so no unk node -- and no fallback run -- starts there (both checked at load); (3) a
            // pre-token that opens a piece follows a document edge (the CSR) or an added-token match, whose token is no fallback token
            w->w_uni_flags.reserve((size_t)n_x + 64);
            pf.begin("unigram_run_offsets");
            launch_unigram_run_offsets(st, grid, t->dt, w->w_ids.as<uint32_t>(), a.offsets, w->w_tok_offsets.as<int64_t>(), n_docs, d_ntok_total, w->w_uni_flags.as<uint8_t>());
            pf.end();
        }
        if (a.want_offsets) out->d_offsets = a.offsets;
        if (a.want_words) out->d_word_ids = a.word_ids;
    }
}

// Enqueue the whole path on `st`.  Inputs and outputs are device pointers.
// d_seq_off / n_seqs: is_pretokenized inputs (InputSequence::PreTokenized, tokenizer/mod.rs:782-795) -- the documents are the WORDS and
// sequence s is the words [d_seq_off[s], d_seq_off[s + 1]); n_seqs < 0: plain documents.
// d_inp_off / n_inputs: a Vec<EncodeInput> that mixes Single and Dual items (tokenizer/mod.rs:225-290, 1337-1356) -- input i is the
// sequences (documents, or sequences of words) [d_inp_off[i], d_inp_off[i + 1]), one or two of them; n_inputs < 0: one kind, per flags.
// The batch is run again, from the caller's own CSR pointers, while its epilogue asks for it (Step::Again).
void run_pipeline(tkamd_tokenizer* t, Workspace* w, const uint8_t* d_text, const int64_t* d_doc_off, int64_t n_docs, int64_t n_bytes,
                  const int64_t* d_seq_off, int64_t n_seqs, uint32_t flags, hipStream_t st, tkamd_device_result* out,
                  const int64_t* d_inp_off = nullptr, int64_t n_inputs = -1) {
    Step step;
    do {
        Batch b{t, w, d_text, d_doc_off, n_docs, n_bytes, d_seq_off, n_seqs, flags, st, out, d_inp_off, n_inputs};
        b.check_request();
        b.zero_batch_state();
        b.validate_inputs();
        if (n_bytes == 0) {
            b.empty_batch();
        } else {
            b.build_x_text();
            b.pretokenize();
            b.run_model();
            b.compact_and_meta();
        }
        step = b.epilogue();
    } while (step == Step::Again);
    HIP_CHECK(hipGetLastError());
}

int read_scalars(tkamd_tokenizer* t, Workspace* w, hipStream_t st, int64_t* n_tok, int64_t* n_pretok);

// Wait for the batch enqueued last; if its <= 16-byte work queue overflowed (ERR_QUEUE_FULL), grow the queue and run the
// same call again on the same stream (the output buffers are sized for the worst case, so the result pointers stay).
int finish_batch(tkamd_tokenizer* t, Workspace* w, hipStream_t st, int64_t* n_tok, int64_t* n_pretok) {
    int bits = read_scalars(t, w, st, n_tok, n_pretok);
    // (rerun_wanted: half the bytes covers every text whose queued pre-tokens have two bytes or more (a word and its separator); one entry
    // per byte covers the rest (runs of one-byte pre-tokens the vocabulary does not know, e.g. punctuation under WordPiece); a speculative
    // batch that met an added token's content is run again with the matching passes -- whatever else its error word says: that run decides)
    while (rerun_wanted(t, w, bits | (w->last_note_added ? NOTE_ADDED_SEEN : 0) | (w->last_note_nfc ? NOTE_NFC_SEEN : 0))) {
        tkamd_device_result again{};
        run_pipeline(t, w, w->last_text, w->last_doc_off, w->last_n_docs, w->last_n_bytes, w->last_seq_off, w->last_n_seqs, w->last_flags, st, &again,
                     w->last_inp_off, w->last_n_inputs);
        if (again.d_ids != w->last_result.d_ids || again.d_tok_offsets != w->last_result.d_tok_offsets ||
            again.d_offsets != w->last_result.d_offsets || again.d_word_ids != w->last_result.d_word_ids || again.d_pad_counts != w->last_result.d_pad_counts || again.d_type_ids != w->last_result.d_type_ids ||
            again.d_enc_docs != w->last_result.d_enc_docs) {
            // (buffers sized from the data -- the padded / overflowing encodings -- may have grown; a device-entry caller already
            // holds the old pointers, the host entry reads w->last_result after this)
            if (w->device_bound) throw HipError("result buffers moved while a batch was run again");
            w->last_result = again;
        }
        bits = read_scalars(t, w, st, n_tok, n_pretok);
    }
    return bits;
}

int read_scalars(tkamd_tokenizer* t, Workspace* w, hipStream_t st, int64_t* n_tok, int64_t* n_pretok) {
    int64_t host[SC_SLOTS];
    const bool census = w->census_pending && w->w_hot_hist.p;      // the batch took a census: its counts come with the scalars, behind the same wait
    if (census) {
        w->h_hot_hist.assign(t->hot_of_slot.size() + 1, 0u);
        HIP_CHECK(hipMemcpyAsync(w->h_hot_hist.data(), w->w_hot_hist.p, w->h_hot_hist.size() * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipMemcpyAsync(host, w->w_scalars.p, sizeof(host), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (census) {
        w->census_pending = false;
        hot_census_read(t, w->h_hot_hist, st);
    }
    int err = *(int*)&host[SC_ERR] & ~NOTE_BITS;             // (notes of the normalizer and of the added tokens' speculation, not errors)
    w->last_note_added = (*(int*)&host[SC_ERR] & NOTE_ADDED_SEEN) != 0;
    w->last_note_nfc = (*(int*)&host[SC_ERR] & NOTE_NFC_SEEN) != 0;
    memcpy(w->last_counters, &host[SC_COUNTERS], sizeof(w->last_counters));
    if (w->last_used_claims && t->claims_pause_len > 0) {
        // the claims' yield, counted by the lookup itself: candidates it looked at and how many of them were another pre-token's word.
        // Fewer than one in four shared: the round trips cost more than the merges they save (tkamd_tokenizer::claims_pause)
        const uint64_t cands = w->last_counters[CNT_CLAIM_CANDS], shared = w->last_counters[CNT_CLAIM_SHARED];
        if (cands >= 32768 && shared * 4 < cands) t->claims_pause = t->claims_pause_len;
    }
    if (n_tok) *n_tok = host[w->last_ntok_slot];
    if (n_pretok) *n_pretok = host[SC_NPRETOK];
    return err;
}

int error_from_bits(int bits) {
    if (bits & ERR_BAD_OFFSETS) return set_error(TKAMD_ERR_INVALID, "doc_offsets is not a monotone CSR over [0, n_bytes]");
    if (bits & ERR_PRETOKEN_TOO_LONG)
        return set_error(TKAMD_ERR_UNSUPPORTED, "pre-tokens longer than 8192 bytes exceed the 1 GiB scratch slab of the global-memory merge path");
    if (bits & ERR_NON_ASCII_NORM)
        return set_error(TKAMD_ERR_UNSUPPORTED, "BertNormalizer strip_accents: a character with a non-zero combining class that survives the Mn filter "
                                                "stands in a run of more than 48 combining characters; NFD's canonical ordering of such a run is not built "
                                                "on the device");
    if (bits & ERR_NFC_SEGMENT)
        return set_error(TKAMD_ERR_UNSUPPORTED, "NFC: a character is followed by more than 48 combining characters (or other characters that may compose with it); "
                                                "the normalization of such a run (NFC, or the NFD of a normalizer chain) is not built on the device");
    if (bits & ERR_ADDED_SPLIT) return set_error(TKAMD_ERR_INVALID, "AddedVocabulary bad split");
    if (bits & ERR_INTERNAL) return set_error(TKAMD_ERR_DEVICE, "internal invariant violated");
    if (bits & ERR_QUEUE_FULL) return set_error(TKAMD_ERR_DEVICE, "work queues still too small after growing them");
    if (bits & ERR_TRUNC_SECOND) return set_error(TKAMD_ERR_INVALID, "Truncation error: Second sequence not provided");
    if (bits & ERR_TRUNC_SHORT) return set_error(TKAMD_ERR_INVALID, "Truncation error: Sequence to truncate too short to respect the provided max_length");
    if (bits & ERR_TRUNC_STRIDE)
        return set_error(TKAMD_ERR_INVALID, "`stride` must be strictly less than `max_len` (note that `max_len` may be shorter than the max length of the "
                                            "original model, as it subtracts the number of special characters");
    if (bits & ERR_TOO_MANY_TOKENS) return set_error(TKAMD_ERR_INVALID, "a truncation leaves more than 2^32 overflowing encodings of one sequence");
    if (bits & ERR_MISSING_UNK) return set_error(TKAMD_ERR_MODEL, "MissingUnkToken: the model needed an unknown token but the vocabulary has none");
    if (bits & ERR_UNK_OOV) return set_error(TKAMD_ERR_MODEL, "UnkTokenOutOfVocabulary: Unk token not found in the vocabulary");
    if (bits & ERR_INPUT_KIND) return set_error(TKAMD_ERR_INVALID, "input_offsets: every input of a mixed batch is one sequence or two");
    return TKAMD_OK;
}

template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const Unsupported& e) {
        return set_error(TKAMD_ERR_UNSUPPORTED, e.what());
    } catch (const Invalid& e) {
        return set_error(TKAMD_ERR_INVALID, e.what());
    } catch (const HipError& e) {
        return set_error(TKAMD_ERR_DEVICE, e.what());
    } catch (const std::bad_alloc&) {
        return set_error(TKAMD_ERR_DEVICE, "out of host memory");
    } catch (const std::exception& e) {
        return set_error(TKAMD_ERR_INVALID, e.what());
    }
}
