// Part of capi.cpp (ONE translation unit: this file is #included there and is not compiled on its own): stage timers, the device tables made at load: upload, the load-time proof of the whole-word table, the short-word and hot tables.

namespace {

// scalars block layout (int64 slots)
enum { SC_NPRETOK = 0, SC_NTOK = 1, SC_ERR = 2 /* int */, SC_NKEPT = 3, SC_PADMAX = 4 /* uint32 */, SC_NSEG = 5, SC_NENC = 6, SC_NCHARS = 8, SC_HUGE_USED = 9, SC_NTOK2 = 10, SC_NPIECE = 11, SC_PLEN = 12,
       SC_COUNTERS = 16 /* uint32[CNT_COUNT] */, SC_SLOTS = 32 };

struct Prof {
    tkamd_tokenizer* t;
    Workspace* w;
    hipStream_t st;
    // TKAMD_TRACE=1: every stage is announced on stderr and waited for -- a faulting kernel is the last name printed
    static bool trace() { static const bool on = getenv("TKAMD_TRACE") != nullptr; return on; }
    void begin(const char* name) {
        if (trace()) fprintf(stderr, "[tkamd] %s ...\n", name);
        if (!t->prof) return;
        StageRec r;
        r.name = name;
        HIP_CHECK(hipEventCreate(&r.a));
        HIP_CHECK(hipEventCreate(&r.b));
        HIP_CHECK(hipEventRecord(r.a, st));
        w->pending.push_back(r);
    }
    void end() {
        if (trace()) { HIP_CHECK(hipStreamSynchronize(st)); fprintf(stderr, "[tkamd]   done\n"); }
        if (!t->prof) return;
        HIP_CHECK(hipEventRecord(w->pending.back().b, st));
    }
};

// (caller holds t->mu)
void drain_profile(tkamd_tokenizer* t, Workspace* w) {
    for (StageRec& r : w->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            auto it = std::find_if(t->acc.begin(), t->acc.end(), [&](const tkamd_stage_time& s) { return r.name == s.name; });
            if (it == t->acc.end()) {
                tkamd_stage_time s{};
                snprintf(s.name, sizeof(s.name), "%s", r.name.c_str());
                t->acc.push_back(s);
                it = t->acc.end() - 1;
            }
            it->ms_total += ms;
            it->launches += 1;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    w->pending.clear();
}

void upload_tables(tkamd_tokenizer* t) {
    HostModel& hm = t->hm;
    upload(t->t_uc1, hm.uc_stage1);
    upload(t->t_uc2, hm.uc_stage2);
    if (!hm.ucc_stage1.empty()) { upload(t->t_ucc1, hm.ucc_stage1); upload(t->t_ucc2, hm.ucc_stage2); }
    std::vector<uint32_t> bid(hm.byte_id, hm.byte_id + 256);
    if (hm.byte_suffix) bid.insert(bid.end(), hm.byte_sfx_id, hm.byte_sfx_id + 256);      // (behind the table itself: DevTables::byte_sfx)
    upload(t->t_byte_id, bid);
    upload(t->t_merges, hm.merge_table);
    upload(t->t_merge_disp, hm.merge_disp);
    // (the two-choice whole-word table stays on the HOST: it is the copy of record build_shortw_table and tkamd_probe_word read; the
    // device probes the short-word table made from it)
    if (hm.decoder != DEC_UNSUPPORTED) {
        upload(t->t_dec_entry, hm.dec_entry, 64);
        upload(t->t_dec_blob, hm.dec_blob, 64);
    }
    upload(t->t_long_blob, hm.long_blob);
    upload(t->t_long_off, hm.long_off);
    upload(t->t_long_id, hm.long_id);
    upload(t->t_long_table, hm.long_table);
    upload(t->t_trie, hm.trie.table);
    {
        std::vector<uint32_t> tpl;
        for (const HostModel::TplPiece& q : hm.pp_pair) { tpl.push_back(q.kind); tpl.push_back(q.id); tpl.push_back(q.type_id); }
        upload(t->t_pp_pair, tpl);
        tpl.clear();
        for (const HostModel::TplPiece& q : hm.pp_pair_plain) { tpl.push_back(q.kind); tpl.push_back(q.id); tpl.push_back(q.type_id); }
        upload(t->t_pp_pair_plain, tpl);
        tpl.clear();
        for (const HostModel::TplPiece& q : hm.pp_single) { tpl.push_back(q.kind); tpl.push_back(q.id); tpl.push_back(q.type_id); }
        upload(t->t_pp_single, tpl);
        tpl.clear();
        for (const HostModel::TplPiece& q : hm.pp_single_plain) { tpl.push_back(q.kind); tpl.push_back(q.id); tpl.push_back(q.type_id); }
        upload(t->t_pp_single_plain, tpl);
    }
    upload(t->t_pp_prefix, hm.pp_prefix);
    upload(t->t_pp_suffix, hm.pp_suffix);
    upload(t->t_pp_prefix_ty, hm.pp_prefix_ty);
    upload(t->t_pp_suffix_ty, hm.pp_suffix_ty);
    upload(t->t_bn1, hm.bn_stage1);
    upload(t->t_bn2, hm.bn_stage2);
    upload(t->t_bn_map, hm.bn_map);
    upload(t->t_nfc1, hm.nfc_stage1);
    upload(t->t_nfc2, hm.nfc_stage2);
    upload(t->t_nfc_map, hm.nfc_map);
    if (hm.norm == NORM_NFKC) {
        upload(t->t_nfk_map, hm.nfk_map);
        upload(t->t_nfk_flat, hm.nfk_flat);
    }
    if (hm.norm == NORM_PRECOMPILED) {
        upload(t->t_pc_units, hm.pc_units);
        upload(t->t_pc_rep, hm.pc_rep);
        upload(t->t_gc1, hm.gc_stage1);
        upload(t->t_gc2, hm.gc_stage2);
    }
    for (int c = 0; c < 2; ++c) {
        upload(t->t_at_blob[c], hm.at[c].blob);
        upload(t->t_at_off[c], hm.at[c].off);
        upload(t->t_at_first[c], hm.at[c].first);
        upload(t->t_at_id[c], hm.at[c].id);
        upload(t->t_at_flags[c], hm.at[c].flags);
    }
    DevTables& d = t->dt;
    d.uc1 = t->t_uc1.as<uint16_t>();
    d.uc2 = t->t_uc2.as<uint8_t>();
    d.byte_id = t->t_byte_id.as<uint32_t>();
    d.byte_sfx = hm.byte_suffix ? d.byte_id + 256 : nullptr;
    d.merges = t->t_merges.as<MergeSlot>();
    d.merge_disp = t->t_merge_disp.as<uint16_t>();
    d.merge_mask = hm.merge_mask;
    d.merge_seed = hm.merge_seed;
    d.newid_affine = hm.merge_newid_affine ? 1u : 0u;
    d.newid_base = hm.merge_newid_base;
    d.merge_bmask = hm.merge_bmask;
    d.word_seed = hm.word_seed;
    d.ignore_merges = hm.ignore_merges ? 1u : 0u;
    d.long_probe_max_len = 0xFFFFFFFFu;
    d.unk_id = hm.unk_id;
    d.has_unk = hm.has_unk ? 1u : 0u;
    d.long_blob = t->t_long_blob.as<uint8_t>();
    d.long_off = t->t_long_off.as<uint32_t>();
    d.long_id = t->t_long_id.as<uint32_t>();
    d.long_table = t->t_long_table.as<uint32_t>();
    d.long_mask = hm.long_mask;
    d.trie = t->t_trie.as<MergeSlot>();
    d.trie_mask = hm.trie.mask;
    d.trie_seed = hm.trie.seed;
    d.max_input_chars = hm.max_input_chars;
    // Unigram (host_model.cpp; unigram_core.hpp)
    d.uni_score = nullptr;
    d.uni_unk_score = hm.uni_unk_score;
    d.uni_is_byte = nullptr;
    d.uni_bytes = hm.uni_bytes ? 1u : 0u;
    d.uni_n_ids = 0u;
    if (hm.model == MODEL_UNIGRAM) {
        upload(t->t_uni_score, hm.uni_score);
        d.uni_score = t->t_uni_score.as<double>();
        if (hm.uni_bytes) {
            std::vector<uint8_t> isb(hm.uni_score.size(), 0);
            for (int b = 0; b < 256; ++b) isb[hm.byte_id[b]] = 1;
            upload(t->t_uni_is_byte, isb);
            d.uni_is_byte = t->t_uni_is_byte.as<uint8_t>();
            d.uni_n_ids = (uint32_t)isb.size();
        }
    }
    // BPE over characters (host_model.cpp: char_id; tables.hpp CB_*)
    d.char_id = nullptr;
    d.cb = 0u;
    if (hm.char_bpe) {
        upload(t->t_char_id, hm.char_id);
        d.char_id = t->t_char_id.as<uint32_t>();
        d.cb = CB_ON | (hm.bpe_prefix.empty() ? 0u : CB_PREFIX) | (hm.bpe_suffix.empty() ? 0u : CB_SUFFIX) | (hm.has_unk ? CB_UNK : 0u) |
               ((hm.unk_configured && !hm.has_unk) ? CB_UNK_MISSING : 0u) | (hm.fuse_unk ? CB_FUSE : 0u) | (hm.byte_fallback ? CB_BYTES : 0u);
    }
}

// Load-time proof of the WORD_DIRECT flag: run the device merge kernel on every <=16-byte vocab
// entry and keep the flag only where merge_word's result is exactly [own id].
void verify_direct_words(tkamd_tokenizer* t) {
    HostModel& hm = t->hm;
    if ((hm.model != MODEL_BPE && hm.model != MODEL_UNIGRAM) || hm.n_words == 0) return;
    std::vector<uint8_t> text;
    std::vector<uint32_t> starts, slot_of;
    for (uint32_t sidx = 0; sidx <= hm.word_mask; ++sidx) {
        const WordSlot& s = hm.word_table[sidx];
        if (s.len == 0) continue;
        uint8_t buf[16];
        memcpy(buf, &s.lo, 8);
        memcpy(buf + 8, &s.hi, 8);
        starts.push_back((uint32_t)text.size());
        slot_of.push_back(sidx);
        text.insert(text.end(), buf, buf + s.len);
    }
    uint32_t P = (uint32_t)starts.size();
    starts.push_back((uint32_t)text.size());
    size_t n = text.size();
    text.resize(n + TKAMD_TEXT_PAD, 0);
    std::vector<uint32_t> items(2 * (size_t)P);                 // QItem {start, length}
    for (uint32_t i = 0; i < P; ++i) { items[2 * i] = starts[i]; items[2 * i + 1] = starts[i + 1] - starts[i]; }
    DevBuf d_text, d_items, d_n, d_rows, d_tmp;
    upload(d_text, text);
    upload(d_items, items);
    std::vector<uint32_t> nn((size_t)NSQ * QCNT_STRIDE, 0u);       // every item in sub-queue 0
    nn[0] = P;
    upload(d_n, nn);
    d_rows.reserve((size_t)P * 16 + 16);
    d_tmp.reserve(n * 4 + 64);
    HIP_CHECK(hipMemset(d_rows.p, 0, (size_t)P * 16));
    const QView v{(QItem*)d_items.p, d_n.as<uint32_t>(), P, 0u};
    if (hm.model == MODEL_UNIGRAM) {
        // Unigram: a whole-word hit is final only if the Viterbi of the word alone yields exactly [id] (with unusual scores a split wins);
        // the Unigram kernel itself says so.  Every word in the <= 16-byte queue, the three others empty; errors (a word that needs an unk
        // the model lacks) do not count, nothing is published
        DevBuf d_errs, d_zero;
        d_errs.reserve(64);
        HIP_CHECK(hipMemset(d_errs.p, 0, 64));
        std::vector<uint32_t> zero((size_t)NSQ * QCNT_STRIDE, 0u);
        upload(d_zero, zero);
        QueuePlan plan{};
        plan.v[0] = v;
        for (int c = 1; c < 4; ++c) plan.v[c] = QView{(QItem*)d_items.p, d_zero.as<uint32_t>(), 1u, 0u};
        launch_unigram_all(nullptr, std::max(1, (int)std::min<uint32_t>(P / 256 + 1, 4096)), 1, t->dt, d_text.as<uint8_t>(), plan, d_rows.p, d_tmp.as<uint32_t>(), nullptr,
                           d_errs.as<int>(), nullptr);
    } else if (hm.char_bpe) {
        // BPE over characters: the kernels that know its start; nothing is published, errors of the vocabulary's own entries do not count
        DevBuf d_errs, d_hl;
        d_errs.reserve(64);
        d_hl.reserve(64);
        HIP_CHECK(hipMemset(d_errs.p, 0, 64));
        HIP_CHECK(hipMemset(d_hl.p, 0, 64));
        DevTables vt = t->dt;
        vt.err = d_errs.as<int>();
        if (vt.newid_affine) launch_bpe_merge(nullptr, t->n_cu, 5, vt, d_text.as<uint8_t>(), v, d_rows.p, d_tmp.as<uint32_t>(), nullptr);
        else launch_bpe_merge_long_only(nullptr, t->n_cu * 2, vt, d_text.as<uint8_t>(), v, d_rows.p, d_tmp.as<uint32_t>(), nullptr, d_hl.as<uint32_t>(), d_hl.as<uint32_t>() + 4);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
    } else
    launch_bpe_merge(nullptr, std::max(1, (int)std::min<uint32_t>(P / 16 + 1, 4096)), 16, t->dt, d_text.as<uint8_t>(), v, d_rows.p, d_tmp.as<uint32_t>(), nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> rows(4 * (size_t)P);
    HIP_CHECK(hipMemcpy(rows.data(), d_rows.p, (size_t)P * 16, hipMemcpyDeviceToHost));
    int nd = 0;
    for (uint32_t i = 0; i < P; ++i) {
        WordSlot& s = hm.word_table[slot_of[i]];
        const uint32_t r0 = rows[4 * (size_t)i];
        const bool one_own = r0 == (s.id | (1u << 28)) ||                                       // row {id | count 1 << 28, ...}: exactly [own id]
                             (r0 == (s.id | (15u << 28)) && rows[4 * (size_t)i + 2] == 1u);   // ... in the long kernel's row form {id | ROW_CNT_MORE << 28, s, count, 0} (results.hip)
        if (one_own) { s.flags |= WORD_DIRECT; ++nd; }
        else s.flags &= ~WORD_DIRECT;
    }
    t->n_direct = nd;
}

// The short-word table (tables.hpp): what pass 2 of the lookup probes.  Built from the 32-byte table (the host's copy of record) once
// its WORD_DIRECT flags are final; same seed (the kernel hashes a key once), its own size.  The table is packed DENSELY -- every line of
// it the lookup has to fetch from beyond the L2 costs (kernels/lookup.hip), and a table of half the size stays in the L2 next to the
// tile's streams where the sparse one was evicted by them: a bucket of k keys fits a given displacement with probability (1 - fill)^k,
// so with 16-bit displacements (65,536 tries) and at most about eight keys a bucket a table 95 % full still places.  The search, in
// this order and deterministic: the power of two at or above words / 0.96 slots (62,000 words and 3,900 both land at 0.95 of
// theirs); the power of two at or above words / 8 buckets, doubled while the placement fails, up to words / 2 (the FEWEST buckets
// that place win: the displacement array is read in front of every probe and should stay small, 16 KB for 50 k words); only then
// twice the slots.  (Measured: DESIGN.md section 4, profiles/dense_tables_*.)
void build_shortw_table(tkamd_tokenizer* t) {
    HostModel& hm = t->hm;
    std::vector<const WordSlot*> ws;
    for (const WordSlot& w : hm.word_table)
        if (w.len) ws.push_back(&w);
    const size_t n = ws.size();
    uint32_t cap = 16;
    while ((uint64_t)cap * 24u < (uint64_t)n * 25u) cap <<= 1;
    uint32_t nb_first = 16;
    while ((size_t)nb_first * 8u < n) nb_first <<= 1;
    std::vector<uint32_t> h1(n), km(n), where(n);
    for (size_t i = 0; i < n; ++i) {
        h1[i] = word_hash1(ws[i]->lo, ws[i]->hi, ws[i]->len, hm.word_seed);
        km[i] = shortw_kmix((uint32_t)ws[i]->lo, (uint32_t)(ws[i]->lo >> 32), (uint32_t)ws[i]->hi, (uint32_t)(ws[i]->hi >> 32));
    }
    // hash-and-displace, the fullest buckets first, each takes the smallest displacement < 65,536 that drops all its words on free slots
    std::vector<uint16_t> disp;
    std::vector<std::vector<uint32_t>> buckets;
    std::vector<uint32_t> order, slots;
    auto place = [&](uint32_t n_buckets) -> bool {
        buckets.assign((size_t)n_buckets, std::vector<uint32_t>());
        for (size_t i = 0; i < n; ++i) buckets[h1[i] & (n_buckets - 1u)].push_back((uint32_t)i);
        order.resize((size_t)n_buckets);
        for (uint32_t b = 0; b < n_buckets; ++b) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return buckets[x].size() > buckets[y].size(); });
        std::vector<uint8_t> used((size_t)cap, 0);
        disp.assign((size_t)n_buckets, 0);
        for (uint32_t b : order) {
            const std::vector<uint32_t>& keys = buckets[b];
            if (keys.empty()) break;
            bool placed = false;
            for (uint32_t d = 0; d < 65536u && !placed; ++d) {
                slots.clear();
                bool clash = false;
                for (uint32_t i : keys) {
                    const uint32_t sl = shortw_slot(h1[i], km[i], d, cap - 1);
                    if (used[sl] || std::find(slots.begin(), slots.end(), sl) != slots.end()) { clash = true; break; }
                    slots.push_back(sl);
                }
                if (clash) continue;
                for (size_t k = 0; k < keys.size(); ++k) { used[slots[k]] = 1; where[keys[k]] = slots[k]; }
                disp[b] = (uint16_t)d;
                placed = true;
            }
            if (!placed) return false;
        }
        return true;
    };
    uint32_t n_buckets = nb_first;
    for (;;) {
        if (place(n_buckets)) break;
        if ((size_t)n_buckets * 2u * 2u <= n) { n_buckets <<= 1; continue; }       // (twice the buckets, while that leaves two words a bucket)
        if (cap >= (1u << 26)) throw Invalid("could not build the short-word hash table");
        cap <<= 1;
        n_buckets = nb_first;
    }
    t->shortw_max_disp = disp.empty() ? 0u : (uint32_t)*std::max_element(disp.begin(), disp.end());
    std::vector<HotSlot> tab(cap, HotSlot{0u, 0u, 0u, 0u});
    std::vector<uint32_t> k3(cap, 0u);
    for (size_t i = 0; i < ws.size(); ++i) {
        const WordSlot* w = ws[i];
        if (w->id > SHORTW_ID_MASK) throw Invalid("token id beyond 24 bits");           // (checked at load already: ids < 2^24)
        tab[where[i]] = HotSlot{(uint32_t)w->lo, (uint32_t)(w->lo >> 32), (uint32_t)w->hi, w->id | (w->len << SHORTW_LEN_SHIFT) | ((w->flags & WORD_DIRECT) ? SHORTW_DIRECT : 0u)};
    }
    for (size_t i = 0; i < ws.size(); ++i) k3[where[i]] = (uint32_t)(ws[i]->hi >> 32);
    t->shortw_of_word.assign(hm.word_table.size(), 0xFFFFFFFFu);      // (the host's side of a census: hot_census_read)
    for (size_t i = 0; i < ws.size(); ++i) t->shortw_of_word[(size_t)(ws[i] - hm.word_table.data())] = where[i];
    upload(t->t_shortw, tab, 64);
    upload(t->t_shortw_k3, k3, 64);
    t->dt.shortw_k3 = t->t_shortw_k3.as<uint32_t>();
    upload(t->t_shortw_disp, disp, 64);
    t->dt.shortw = t->t_shortw.p;
    t->dt.shortw_disp = t->t_shortw_disp.as<uint16_t>();
    t->dt.shortw_mask = cap - 1;
    t->dt.shortw_bmask = n_buckets - 1u;
}

// Hot-word table of the lookup kernel: settled words of <= 12 bytes, hash-and-displace (tables.hpp; the builder: hot_table_core.hpp).
// "Settled" = a hit needs no further work: every word for WordLevel / WordPiece / ignore_merges, the WORD_DIRECT ones for
// byte-level BPE.  At load every word weighs the same and the lowest ids win (trainers hand out ids in frequency order -- true of tokens);
// a census of the handle's own text (kernels/lookup.hip k_hot_census) then weighs the words by how often they stand as whole pre-tokens,
// and hot_census_read below builds the table again from those weights.  A word that is not in the table stays reachable through the
// short-word table: what the table holds never changes a result.
void hot_install(tkamd_tokenizer* t, const HotTableBuild& b) {
    t->n_hot = b.n_hot;
    t->hot_blob = b.blob;
    t->hot_member.assign(t->hot_words.size(), 0);
    for (uint32_t i : b.placed) t->hot_member[i] = 1;
}

void build_hot_table(tkamd_tokenizer* t) {
    HostModel& hm = t->hm;
    const bool all_final = (hm.model != MODEL_BPE && hm.model != MODEL_UNIGRAM) || hm.ignore_merges;
    t->hot_words.clear();
    t->hot_of_slot.assign((size_t)t->dt.shortw_mask + 1u, -1);
    for (size_t i = 0; i < hm.word_table.size(); ++i) {
        const WordSlot& w = hm.word_table[i];
        if (!(w.len && w.len <= (uint32_t)HOT_MAX_KEY && (all_final || (w.flags & WORD_DIRECT)))) continue;
        const uint32_t slot = i < t->shortw_of_word.size() ? t->shortw_of_word[i] : 0xFFFFFFFFu;
        if (slot < t->hot_of_slot.size()) t->hot_of_slot[slot] = (int32_t)t->hot_words.size();
        t->hot_words.push_back(HotWord{(uint32_t)w.lo, (uint32_t)(w.lo >> 32), (uint32_t)w.hi, w.len, w.id, 0ull});
    }
    const HotTableBuild b = build_hot_table_core(t->hot_words, (uint32_t)HOT_SLOTS, hm.word_seed);
    hot_install(t, b);
    upload(t->t_hot, b.blob);
    t->hot_cur = t->t_hot.p;
}

// The synchronisation of a batch that took a census (read_scalars, behind its wait): h = the counts by short-word slot, then the sampled
// pre-tokens.  Nothing the device wrote is trusted: a count is taken only for a slot of the host's own table whose word is <= 12 bytes and
// settled by the rule above (hot_of_slot) -- a word that is not could change ids from inside the hot table -- and the rates are
// clamped.  The table the counts select replaces the one in use only if it would have settled HOT_GAIN more of the sample: text whose
// words stay what they were settles after one rebuild.
void hot_census_read(tkamd_tokenizer* t, const std::vector<uint32_t>& h, hipStream_t st) {
    std::lock_guard<std::mutex> lk(t->mu);
    const size_t n_slots = t->hot_of_slot.size();
    if (h.size() != n_slots + 1) return;
    const uint64_t total = h[n_slots];
    if (total == 0) return;
    std::vector<HotWord> words = t->hot_words;
    t->hot_counts.assign(words.size(), 0u);
    uint64_t cur = 0;
    for (size_t s = 0; s < n_slots; ++s) {
        if (!h[s] || t->hot_of_slot[s] < 0) continue;
        const size_t e = (size_t)t->hot_of_slot[s];
        words[e].weight = h[s];
        t->hot_counts[e] = h[s];
        if (t->hot_member[e]) cur += h[s];
    }
    const HotTableBuild b = build_hot_table_core(words, (uint32_t)HOT_SLOTS, t->hm.word_seed);
    auto rate = [&](uint64_t x) { return (uint32_t)(std::min(x, total) * 10000ull / total); };
    t->hot_sample = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
    t->hot_rate_cur = rate(cur);
    t->hot_rate_sel = rate(b.weight_placed);
    if (t->hot_rate_sel < t->hot_rate_cur + (uint32_t)(HOT_GAIN * 10000.0) || t->hot_ring.size() + 1 >= HOT_RING) return;
    // a buffer of its own, complete before any launch can be given its address
    std::unique_ptr<DevBuf> nb(new DevBuf());
    nb->reserve(b.blob.size());
    HIP_CHECK(hipMemcpyAsync(nb->p, b.blob.data(), b.blob.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    hot_install(t, b);
    t->hot_cur = nb->p;
    t->hot_ring.push_back(std::move(nb));
    ++t->hot_gen;
}
