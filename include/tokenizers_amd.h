/*
 * tokenizers_amd.h -- C ABI of the MI355X-native encode_batch path.
 *
 * This is the drop-in boundary for ONE hot path of huggingface/tokenizers:
 *   TokenizerImpl::encode_batch / encode_batch_char_offsets / encode_batch_fast
 *   (reference: tokenizers/src/tokenizer/mod.rs:1337-1401), i.e. per document
 *   extract_and_normalize -> PreTokenizer::pre_tokenize -> Model::tokenize ->
 *   PreTokenizedString::into_encoding (mod.rs:762-805, pre_tokenizer.rs:198-263).
 *
 * The reference has no FFI for this path (its plugin API is Rust traits,
 * tokenizer/mod.rs:56-207), so the entry points below are what a Rust
 * `extern "C"` block / a ctypes stub would bind.  Plain
 * pointers and sizes only; no C++ / torch types; nothing throws across the ABI.
 *
 * Data model (replaces Vec<EncodeInput> in, Vec<Encoding> out):
 *   in : one contiguous UTF-8 buffer `text` + CSR `doc_offsets[n_docs+1]`
 *        (document d = text[doc_offsets[d] .. doc_offsets[d+1]) ).
 *   out: CSR token arrays: ids[n_tokens] (u32) + tok_offsets[n_docs+1] (i64),
 *        and, when requested, per-token (start,end) offsets relative to the
 *        document and per-token word ids (= pre-token index in the document,
 *        pre_tokenizer.rs:252-256).
 *   These are the fields of `Encoding` (tokenizer/encoding.rs:11-31) that
 *   carry information; type_ids / attention_mask / special_tokens_mask follow
 *   from the special-token layout (tkamd_tokenizer_specials) and the padding
 *   counts (tkamd_batch_pad_counts) and are synthesised by the host shim.
 *   A `truncation` / `padding` section of tokenizer.json is honoured
 *   (utils/truncation.rs, utils/padding.rs); with TKAMD_WANT_OVERFLOW the
 *   `overflowing` encodings a truncation leaves behind (Encoding::truncate,
 *   tokenizer/encoding.rs:307-395) are further encodings of the result.
 *   EncodeInput::Dual (pairs), InputSequence::PreTokenized (lists of words) and
 *   batches that mix single sequences and pairs (tokenizer/mod.rs:225-290) are
 *   the same buffers with one more CSR: TKAMD_PAIRS, tkamd_encode_batch_words,
 *   tkamd_encode_batch_mixed below.
 */
#ifndef TOKENIZERS_AMD_H
#define TOKENIZERS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (Result<_, Box<dyn Error>> at tokenizer/mod.rs:51-52) ---- */
#define TKAMD_OK              0
#define TKAMD_ERR_INVALID    -1   /* bad argument / malformed tokenizer.json                    */
#define TKAMD_ERR_UNSUPPORTED -2  /* tokenizer.json uses a component outside this hot path     */
#define TKAMD_ERR_DEVICE     -3   /* HIP runtime error (no device, OOM, launch failure)        */
#define TKAMD_ERR_MODEL      -4   /* model error the reference raises too (e.g. MissingUnkToken,
                                     models/wordlevel/mod.rs:175-177, wordpiece/mod.rs:229-232) */

/* ---- encode flags (OffsetType at tokenizer/pre_tokenizer.rs:10-17) ---- */
#define TKAMD_OFFSETS_NONE   0u   /* encode_batch_fast          (mod.rs:1382-1401)             */
#define TKAMD_OFFSETS_BYTE   1u   /* Rust encode_batch          (mod.rs:1337-1356)             */
#define TKAMD_OFFSETS_CHAR   2u   /* encode_batch_char_offsets  (mod.rs:1360-1379; Python)     */
#define TKAMD_OFFSETS_MASK   3u
#define TKAMD_WANT_WORD_IDS  4u   /* also produce Encoding.words                               */
#define TKAMD_ADD_SPECIAL    8u   /* add_special_tokens=true: PostProcessor::process for a single sequence
                                     (processors/bert.rs:51-120, roberta.rs, template.rs:544-590): special ids
                                     around every document, offsets (0,0), word id 0xFFFFFFFF (None)          */

#define TKAMD_PAIRS          16u   /* EncodeInput::Dual (tokenizer/mod.rs:871-889): documents 2i and 2i+1 are sequence A and B of
                                     encoding i (n_docs must be even); the result holds n_docs / 2 encodings: the pair is
                                     truncated together, laid out by the post-processor's pair template (type ids), padded  */

#define TKAMD_WANT_OVERFLOW   32u   /* Encoding.overflowing: with a `truncation` section, what a single sequence loses to the cut comes back as
                                     further encodings -- windows of max_length tokens (less the special tokens) that share `stride` tokens
                                     with their neighbour (tokenizer/encoding.rs:307-395), each with the same special tokens and padding as
                                     the truncated encoding (processors/bert.rs:88-125, encoding.rs:466-469).  The result then holds
                                     n_encodings >= n_docs encodings: every document's own followed by its overflowing ones in the
                                     reference's order; tkamd_batch_encoding_docs / d_enc_docs name the document of each.  A PAIR
                                     leaves every combination of its two sequences' windows (Encoding::merge_with, encoding.rs:408-432):
                                     with F the sequence the template names first, S the other, f_1.. / s_1.. their overflowing
                                     windows, the pair's encodings are F+S; then for every f_x: f_x+S, f_x+s_1, f_x+s_2 ..; then
                                     F+s_1, F+s_2 .. -- the reference's flat `overflowing` list (it also hangs f_x+s_* below f_x+S and
                                     f_*+s_y below F+s_y as nested lists: the same encodings; tkamd_batch_encoding_parts names the
                                     windows so a binding can rebuild them).  Ignored without a `truncation` section.                */

/* Readable slack the caller must leave after text[n_bytes] for the device entry
 * points (kernels read whole 16-byte words).  The host entry pads internally. */
#define TKAMD_NO_SPECULATION  64u   /* A tokenizer with added tokens runs a batch as if its text held none (natural text holds no special token: one
                                     detection pass instead of the matching passes of AddedVocabulary::extract_and_normalize,
                                     added_vocabulary.rs:523-564); a batch whose text does hold the content of one is run again with the matching
                                     passes when the call synchronises (the host entries before they return, the device entry in
                                     tkamd_device_sync) -- results are the reference's either way.  A caller of the device entry that
                                     consumes the results stream-ordered behind the call, WITHOUT tkamd_device_sync in between, sets this
                                     flag: the matching passes run outright.  The same holds for a tokenizer with an NFC normalizer: a
                                     batch runs over the text as it came behind an exact quick check and is run again through the
                                     normalizer when the call synchronises and the check failed; with this flag it is normalized outright.
                                     Without the flag AND without tkamd_device_sync a text that is not NFC would be encoded un-normalized. */
#define TKAMD_TEXT_PAD 64

typedef struct tkamd_tokenizer tkamd_tokenizer;  /* immutable after creation; owns device tables */
typedef struct tkamd_batch     tkamd_batch;      /* one encode_batch result (host copies)        */

/* What was recognised in tokenizer.json (for the host shim / diagnostics). */
typedef struct tkamd_info {
    int32_t model;          /* 1 BPE, 2 WordPiece, 3 WordLevel, 4 Unigram                       */
    int32_t pre_tokenizer;  /* 1 ByteLevel(GPT-2 regex; also that regex spelled as a Split), 2 Split(a pattern of the tiktoken family:
                               Llama-3 / cl100k, Qwen2, o200k, tekken ...; pre_tokenizers/split.rs:76-105) + ByteLevel, 3 Whitespace,
                               4 WhitespaceSplit, 5 BertPreTokenizer, 6 ByteLevel(use_regex=false), 7 the U+2581 front of SentencePiece-style BPE,
                               8 the chain of three Splits of DeepSeek-V3 / R1 + ByteLevel(use_regex=false),
                               9 Sequence[Digits, ByteLevel(GPT-2 regex)]: StarCoder / StarCoder2 / SantaCoder, Granite code, Command-R,
                               10 Sequence[Split(the CLIP pattern, Removed, inverted), ByteLevel]: CLIP, the text encoders of Stable Diffusion,
                               11 Sequence[Split(BLOOM's pattern, Isolated), ByteLevel(use_regex=false)]: BLOOM / BLOOMZ.
                               (7 also: Split(String " ", MergedWithPrevious) behind the U+2581 normalizers, where it is inert: Gemma-2 / Gemma-3) */
    int32_t normalizer;     /* 0 none, 1 BertNormalizer, 2 the U+2581 normalizers, 3 NFC, 4 Precompiled,
                               5 NFD / Lowercase / StripAccents, alone or chained in a Sequence, 6 NFKC,
                               7 Sequence[NFC, Replace(Regex "\\s+" -> " "), Lowercase] (with or without the Replace) of the CLIP files */
    int32_t vocab_size;
    int32_t n_merges;
    int32_t add_prefix_space;
    int32_t ignore_merges;
    int32_t n_added_tokens; /* special/added tokens registered in the JSON                       */
    int32_t device;         /* HIP device ordinal, -1 = host-only handle (no kernels)           */
    int32_t n_direct_words; /* entries of the whole-word table proven merge-stable (see DESIGN)  */
    int32_t truncation;         /* max_length of the `truncation` section, -1 = none (utils/truncation.rs)          */
    int32_t padding;            /* 0 none, 1 pad on the right, 2 on the left (utils/padding.rs)                       */
    int32_t pad_id;
    int32_t pad_type_id;
    int32_t word_disp_entries;  /* always 0 since round 4 (the whole-word table is a two-choice table without displacements);
                                   the field keeps the struct's layout                                                */
    int32_t merge_disp_entries; /* displacement entries of the merge table's perfect hash (> 16384: the kernels read them
                                   from global memory instead of their LDS copy)                                      */
} tkamd_info;

/* Replaces Tokenizer::from_file / from_str (tokenizer/mod.rs:468-472, serialization.rs:104-171).
 * `device` >= 0: build HBM-resident tables on that HIP device.  `device` == -1: parse and build
 * host tables only (no GPU needed; encode calls then fail with TKAMD_ERR_DEVICE). */
int tkamd_tokenizer_from_json(const char* json, size_t json_len, int device, tkamd_tokenizer** out);
void tkamd_tokenizer_free(tkamd_tokenizer* tok);
int tkamd_tokenizer_info(const tkamd_tokenizer* tok, tkamd_info* info);

/* ---- one call, every GPU ------------------------------------------------------------------------
 * TokenizerImpl::encode_batch is ONE call that uses every parallel resource of the machine: it maps `encode` over the inputs on the
 * Rayon pool (tokenizer/mod.rs:1345-1348, utils/parallelism.rs:85-106).  The counterpart here: a handle made over a LIST of devices
 * replicates the tables on each (<= 5 MB) and the host entries (tkamd_encode_batch, tkamd_encode_batch_words) then cut every batch
 * into one contiguous, byte-balanced run of documents per device -- one host thread and one stream per device, each shard's text
 * going up its own PCIe link -- and return ONE result in document order.  How the shards' results meet is the handle's collect mode:
 *   TKAMD_COLLECT_HOST       every device copies its ids straight into its slice of the one pinned result (no collective): the
 *                            default; N links carry the result.
 *   TKAMD_COLLECT_ROOT_P2P   the peers push their shards into one buffer on devices[0] over xGMI (hipMemcpyPeerAsync), one D2H.
 *   TKAMD_COLLECT_ROOT_RCCL  the same gather with RCCL: ncclSend on every peer, ncclRecv at the displacement on devices[0]
 *                            (RCCL has no gatherv; librccl.so is opened at first use) -- the reference's `collect()` of the
 *                            Vec<Encoding> as a collective, for consumers that want the result on one GPU.
 * A device may be named more than once (two shards then share a GPU: how the sharded path is tested on a one-GPU box; RCCL needs
 * distinct devices).  n_devices == 0: the list comes from the environment, TOKENIZERS_GPU_DEVICES = "all" | "0,2,3" (unset: device
 * 0).  BatchLongest padding couples the documents of a batch through one number -- the longest encoding: the shards exchange theirs and
 * pad to the batch's (utils/padding.rs:55-63).  TKAMD_WANT_OVERFLOW (a shard's encodings are counted when its kernels are done, its
 * document indices rebased) and mixed batches (cut between inputs) are sharded like the rest; a batch of
 * less than 1 MB per device runs on devices[0] alone (TKAMD_SHARD_MIN_KB, read when the handle is made).  The device-buffer entries and decode_batch run on devices[0]. */
#define TKAMD_COLLECT_HOST      0
#define TKAMD_COLLECT_ROOT_P2P  1
#define TKAMD_COLLECT_ROOT_RCCL 2
int tkamd_tokenizer_from_json_devices(const char* json, size_t json_len, const int* devices, int n_devices, tkamd_tokenizer** out);
int tkamd_tokenizer_set_collect(tkamd_tokenizer* tok, int mode);
/* devices[0 .. *n) of the handle (1 entry for a single-device handle, 0 for a host-only one). */
int tkamd_tokenizer_devices(const tkamd_tokenizer* tok, int* devices, int cap, int* n);
/* The last sharded host-entry call: per device of the handle, the bytes of its shard and the wall milliseconds its host thread was
 * busy (H2D + kernels + its part of the collect) -- BASELINE configs[4]'s "per-GPU busy time imbalance (max / mean)". */
int tkamd_shard_stats(const tkamd_tokenizer* tok, int64_t* shard_bytes, double* busy_ms, int cap, int* n);

/* Special-token layout of the post-processor for a single sequence: ids inserted before / after every document
 * when TKAMD_ADD_SPECIAL is set.  Returns TKAMD_ERR_UNSUPPORTED if the post-processor is outside the path. */
int tkamd_tokenizer_specials(const tkamd_tokenizer* tok, uint32_t* prefix_ids, int32_t* n_prefix, uint32_t* suffix_ids,
                             int32_t* n_suffix, int32_t cap);

/* The same for a pair (TKAMD_PAIRS): the post-processor's pair template as pieces of three values each -- kind (0 sequence A,
 * 1 sequence B, 2 special token), token id (kind 2), type id -- in output order; with_specials = 0: the layout without
 * add_special_tokens (A then B, PostProcessor::default_process).  *n_pieces = number of pieces (written even beyond cap). */
int tkamd_tokenizer_pair_template(const tkamd_tokenizer* tok, int with_specials, uint32_t* pieces, int32_t cap, int32_t* n_pieces);

/* Thread-local message of the last failing call on this thread (error.rs:26-31 maps
 * the reference's error to `Exception(str(e))`; the shim does the same with this). */
const char* tkamd_last_error(void);

/* ---- host-buffer entry: H2D + kernels + D2H -------------------------------------------------
 * Replaces TokenizerImpl::encode_batch{,_char_offsets,_fast}(inputs, add_special_tokens=false)
 * for Single(Raw) inputs.  `text`/`doc_offsets` are borrowed for the call.  The result is owned
 * by the library until tkamd_batch_free. */
int tkamd_encode_batch(tkamd_tokenizer* tok, const uint8_t* text, const int64_t* doc_offsets,
                       int64_t n_docs, uint32_t flags, tkamd_batch** out);

/* is_pretokenized = true (InputSequence::PreTokenized, tokenizer/mod.rs:225-290; encode_single_sequence :782-795): every input
 * sequence is a list of words.  The reference encodes each word on its own -- AddedVocabulary, normalizer, pre-tokenizer, model:
 * a ByteLevel add_prefix_space therefore applies to every word, and offsets are relative to the WORD -- and merges the
 * encodings with word_ids = the word's index in its sequence; truncation, special tokens and padding then see one encoding per
 * sequence.  `text` is the concatenation of all words, word_offsets[n_words + 1] their byte CSR, seq_offsets[n_seqs + 1] the CSR of
 * the sequences over the words.  With TKAMD_PAIRS sequences 2i and 2i + 1 are sequence A and B of encoding i.  The result holds one
 * encoding per sequence (or pair). */
int tkamd_encode_batch_words(tkamd_tokenizer* tok, const uint8_t* text, const int64_t* word_offsets, int64_t n_words,
                             const int64_t* seq_offsets, int64_t n_seqs, uint32_t flags, tkamd_batch** out);

/* One call for a Vec<EncodeInput> that mixes EncodeInput::Single and EncodeInput::Dual items (tokenizer/mod.rs:225-290; encode_batch
 * maps `encode` over them, :1337-1356, and pads the lot together, utils/padding.rs:50-81).  The sequences of the batch are laid out as
 * for tkamd_encode_batch (seq_offsets == NULL: `text` + doc_offsets[n_docs + 1], a sequence is a document) or as for
 * tkamd_encode_batch_words (seq_offsets[n_seqs + 1] over the words word_offsets = doc_offsets[n_docs + 1]); input i is the sequences
 * [input_offsets[i], input_offsets[i + 1]): one -- a single sequence -- or two -- sequence A and B of a pair.  Every input is cut,
 * laid out by the post-processor's template of ITS kind (n_added_tokens(is_pair) taken off max_length, mod.rs:1270-1284) and the batch
 * is padded as one (BatchLongest over every input).  TKAMD_PAIRS must not be set.  The result holds one encoding per input (plus the
 * overflowing ones with TKAMD_WANT_OVERFLOW; tkamd_batch_encoding_parts then gives (window, 0) for a single sequence); type ids and
 * sequence ids are written for every token.  A batch that turns out to hold one kind only is handed to the entry of that kind; a
 * mixed one runs as one slice (a multi-device handle: one shard per device, cut between inputs).  TKAMD_ERR_INVALID for an input of no or more than two sequences. */
int tkamd_encode_batch_mixed(tkamd_tokenizer* tok, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                             const int64_t* seq_offsets, int64_t n_seqs, const int64_t* input_offsets, int64_t n_inputs,
                             uint32_t flags, tkamd_batch** out);

/* tkamd_encode_batch for a caller that is still FILLING `text` while the call runs.  The reference's Python binding turns every
 * input into an owned Rust String first and encodes afterwards (bindings/python/src/tokenizer.rs:1312-1338: the extraction loop,
 * then py.allow_threads around encode_batch); a binding of this library packs its strings into one buffer anyway -- with this entry
 * the packing of the batch's tail overlaps the H2D copy and the kernels of its head.  doc_offsets[0 .. n_docs] is complete on entry;
 * bytes [0, *ready_bytes) of `text` are valid, *ready_bytes only grows (written with release semantics by the caller's packing
 * threads, read with acquire semantics here) and reaches doc_offsets[n_docs].  The call never reads a byte it has not seen announced.
 * `consumed(user)`, if not NULL, is called once from the calling thread as soon as the call has seen *ready_bytes at its final value
 * (the caller's source objects are no longer needed: a Python binding releases the GIL there) -- also on every error path that
 * waited that long; a call that fails before has not called it.  A producer that cannot finish stores a NEGATIVE value in
 * *ready_bytes: the call stops waiting, calls `consumed` and fails with TKAMD_ERR_INVALID (without that signal a producer that
 * dies leaves the call waiting for ever).  pace == NULL: tkamd_encode_batch. */
typedef struct tkamd_pace {
    const int64_t* ready_bytes;
    void (*consumed)(void* user);
    void* user;
} tkamd_pace;
int tkamd_encode_batch_paced(tkamd_tokenizer* tok, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, uint32_t flags,
                             const tkamd_pace* pace, tkamd_batch** out);

int64_t         tkamd_batch_n_docs(const tkamd_batch* b);       /* encodings in the result (= documents / sequences / pairs, plus the
                                                                   overflowing encodings with TKAMD_WANT_OVERFLOW)              */
int64_t         tkamd_batch_n_tokens(const tkamd_batch* b);
const uint32_t* tkamd_batch_ids(const tkamd_batch* b);          /* [n_tokens]                   */
const int64_t*  tkamd_batch_tok_offsets(const tkamd_batch* b);  /* [n_docs+1] CSR into ids      */
const uint32_t* tkamd_batch_offsets(const tkamd_batch* b);      /* [n_tokens][2] or NULL        */
const uint32_t* tkamd_batch_word_ids(const tkamd_batch* b);     /* [n_tokens] or NULL           */
const uint8_t*  tkamd_batch_type_ids(const tkamd_batch* b);     /* [n_tokens] Encoding.type_ids (pairs; single sequences under a TemplateProcessing with type ids), or NULL: 0, pad_type_id on padding */
const uint8_t*  tkamd_batch_sequence_ids(const tkamd_batch* b); /* [n_tokens] 0 / 1 = token of sequence A / B, 2 = special token, 3 = padding, or NULL
                                                                   (single sequences: derived from tkamd_tokenizer_specials and the pad counts)      */
const uint32_t* tkamd_batch_pad_counts(const tkamd_batch* b);   /* [n_docs] padding tokens of each encoding (at the side
                                                                   tkamd_info.padding names), NULL without a `padding` section:
                                                                   attention_mask = 0, special_tokens_mask = 1 on them      */
const uint32_t* tkamd_batch_encoding_docs(const tkamd_batch* b);/* [n_docs] TKAMD_WANT_OVERFLOW with a `truncation` section: the document
                                                                   (sequence) every encoding belongs to, ascending -- a document's
                                                                   first encoding is the truncated one, the rest are its
                                                                   Encoding.overflowing in order; NULL otherwise                */
const uint32_t* tkamd_batch_encoding_parts(const tkamd_batch* b);/* [n_docs][2] TKAMD_WANT_OVERFLOW | TKAMD_PAIRS: which window of sequence A
                                                                   and of sequence B every encoding combines (0 = the truncated
                                                                   sequence itself, 1.. = its overflowing windows); NULL otherwise */
void            tkamd_batch_free(tkamd_batch* b);

/* ---- page-locked memory for the caller's side of the host entry ---------------------------------
 * tkamd_encode_batch takes `text` / `doc_offsets` from any host memory; from pageable memory the runtime stages the copy through
 * its own bounce buffers (about half the link's rate, and the calling thread does the copying).  The binding has to pack the
 * documents into one buffer anyway: packing them into a block from here costs nothing extra and lets the H2D
 * copies run as plain DMA.  Blocks are portable across the devices of a multi-device handle; free them with tkamd_pinned_free
 * (never free()).  Fails with TKAMD_ERR_DEVICE where no HIP device exists. */
int  tkamd_pinned_alloc(size_t bytes, void** out);
void tkamd_pinned_free(void* p);

/* ---- device-buffer entry: inputs already resident in HBM, outputs stay in HBM ---------------
 * Enqueues the whole path on `hip_stream` (a hipStream_t, NULL = default stream) and returns
 * without synchronising.  The output pointers refer to the handle's workspace and stay valid
 * until the next encode call on the same handle.  d_n_tokens[0] holds the token count once the
 * stream has drained; tkamd_device_sync() waits for it and returns it. */
typedef struct tkamd_device_result {
    const uint32_t* d_ids;          /* [n_tokens]                                               */
    const int64_t*  d_tok_offsets;  /* [n_docs+1]                                               */
    const uint32_t* d_offsets;      /* [n_tokens][2] or NULL                                    */
    const uint32_t* d_word_ids;     /* [n_tokens] or NULL                                       */
    const int64_t*  d_n_tokens;     /* [1]                                                      */
    const int64_t*  d_n_pretokens;  /* [1] number of pre-tokens (splits) in the batch           */
    const uint32_t* d_pad_counts;   /* [n_docs] padding tokens per encoding, or NULL            */
    const uint8_t*  d_type_ids;     /* TKAMD_PAIRS, or a single template with type ids: [n_tokens], else NULL */
    const uint8_t*  d_seq_ids;      /* TKAMD_PAIRS: [n_tokens] 0 / 1 / 2 special / 3 padding    */
    const uint32_t* d_enc_docs;     /* TKAMD_WANT_OVERFLOW (with a `truncation` section): [n_encodings] document of every encoding, else NULL;
                                       d_tok_offsets / d_pad_counts then have n_encodings (+ 1) entries                                        */
    const int64_t*  d_n_encodings;  /* [1] with d_enc_docs, else NULL (the call itself waits for this count: it sizes the result)              */
    const uint32_t* d_enc_parts;    /* TKAMD_WANT_OVERFLOW | TKAMD_PAIRS: [n_encodings][2] window of A / of B, else NULL                       */
    int64_t         ids_capacity;   /* an upper bound of n_tokens known when the call returns (before the stream has drained): a consumer on
                                       the same stream may treat d_ids (and the other per-token arrays) as arrays of this many elements and
                                       read the count from d_n_tokens on the device.  0: no such bound (the padded / overflowing encodings of
                                       a `truncation` / `padding` section are sized from the data)                                            */
} tkamd_device_result;

int tkamd_encode_batch_device(tkamd_tokenizer* tok, const uint8_t* d_text, const int64_t* d_doc_offsets,
                              int64_t n_docs, int64_t n_bytes, uint32_t flags, void* hip_stream,
                              tkamd_device_result* out);
/* tkamd_encode_batch_words on device-resident buffers (d_seq_offsets: [n_seqs + 1] int64 in HBM as well). */
int tkamd_encode_batch_words_device(tkamd_tokenizer* tok, const uint8_t* d_text, const int64_t* d_word_offsets, int64_t n_words,
                                    int64_t n_bytes, const int64_t* d_seq_offsets, int64_t n_seqs, uint32_t flags, void* hip_stream,
                                    tkamd_device_result* out);
int tkamd_device_sync(tkamd_tokenizer* tok, void* hip_stream, int64_t* n_tokens, int64_t* n_pretokens);

/* ---- dense entry: text in HBM in, padded [n_rows, width] arrays in the CALLER's HBM out ---------------------------
 * What a model's forward pass reads -- transformers' input_ids / attention_mask / token_type_ids / special_tokens_mask / offset_mapping
 * / word_ids -- written by one more stage behind the epilogue (kernels/dense.hip) into memory the caller owns (a torch tensor's
 * data_ptr), every array as int64 or every array as int32.  tkamd_encode_batch_device_dense is tkamd_encode_batch_device with
 * TKAMD_WANT_DENSE | TKAMD_NO_SPECULATION set by the call itself: flags takes the offsets mode, TKAMD_WANT_WORD_IDS, TKAMD_ADD_SPECIAL
 * and TKAMD_PAIRS (documents 2i / 2i + 1 -> row i).  The call only enqueues: no synchronisation, no copy to the host, and after a first
 * call of the same size no allocation; the arrays are final when `hip_stream` reaches them.  The one exception is a batch whose work
 * queue overflowed (natural text does not): tkamd_device_sync runs it again, as for every device call, and the re-run fills the same
 * arrays -- `d_text`, `d_doc_offsets` and the arrays of `dst` must stay alive until the batch has been synchronised or the next call on
 * the stream was made.  `out` is filled as by tkamd_encode_batch_device (the padded CSR in the workspace; ids_capacity = n_rows * width).
 *   input_ids           the ids, pad_id on padding
 *   attention_mask      0 on padding, else 1
 *   token_type_ids      the template's type ids (pairs, typed single templates); else 0, pad_type_id on padding
 *   special_tokens_mask 1 on special tokens and on padding
 *   offsets             [n_rows][width][2] (start, end) in the call's offsets mode -- refused with TKAMD_OFFSETS_NONE; (0, 0) on special
 *                       tokens and padding
 *   word_ids            the word index, -1 for none -- refused without TKAMD_WANT_WORD_IDS
 * The row width must be known before the call, so the handle needs a `truncation` section and a `padding` section with a Fixed
 * strategy: width = its length rounded up to pad_to_multiple_of, max_length <= width, and with TKAMD_ADD_SPECIAL max_length must be at
 * least the number of special tokens the (single or pair) template adds.  tkamd_dense_width answers that width for `flags`
 * (TKAMD_ADD_SPECIAL and TKAMD_PAIRS matter) or fails with TKAMD_ERR_INVALID naming the missing piece.  Refused up front, with
 * TKAMD_ERR_INVALID and before any device work: TKAMD_WANT_OVERFLOW (the number of rows would be known on the device only),
 * dst->n_rows != n_docs (n_docs / 2 for pairs), dst->width != that width, a multi-device handle.  Pre-tokenized and mixed inputs have
 * no dense entry.  TKAMD_WANT_DENSE itself is refused by every other entry. */
#define TKAMD_WANT_DENSE 128u
#define TKAMD_DENSE_I32 1u
typedef struct tkamd_dense_out {
    void *input_ids, *attention_mask, *token_type_ids, *special_tokens_mask, *offsets, *word_ids;  /* device; all but input_ids may be NULL */
    int64_t n_rows, width;
    uint32_t dtype_flags;     /* 0: int64 elements, TKAMD_DENSE_I32: int32 */
} tkamd_dense_out;
int tkamd_dense_width(const tkamd_tokenizer* tok, uint32_t flags, int64_t* width);
int tkamd_encode_batch_device_dense(tkamd_tokenizer* tok, const uint8_t* d_text, const int64_t* d_doc_offsets, int64_t n_docs, int64_t n_bytes,
                                    uint32_t flags, void* hip_stream, const tkamd_dense_out* dst, tkamd_device_result* out);

/* ---- decode_batch: token ids -> text -----------------------------------------------------------
 * Replaces Tokenizer::decode_batch (tokenizer/mod.rs:1404-1416) = map of Tokenizer::decode (mod.rs:935-953):
 * id -> token string (added vocabulary first, added_vocabulary.rs:239-246; ids without a token are dropped),
 * specials dropped when TKAMD_SKIP_SPECIAL (skip_special_tokens), then the `decoder` section:
 * ByteLevel (pre_tokenizers/byte_level.rs:155-171), WordPiece (decoders/wordpiece.rs:46-64), BPEDecoder (decoders/bpe.rs:26-39),
 * ByteFallback (byte_fallback.rs:27-67), Fuse (fuse.rs:24-29), Replace with a literal pattern (normalizers/replace.rs:88-106), Strip
 * (strip.rs:27-60), a Sequence (sequence.rs:26-33) of the shape [Replace*, Strip*, ByteFallback?, Fuse?, Strip(c, <= 1, 0)?], CTC
 * (ctc.rs:45-63) or none (join with " ").  Other decoders / shapes -> TKAMD_ERR_UNSUPPORTED.  The result is the raw byte string per sequence; the
 * ByteLevel decoder's String::from_utf8_lossy (byte_level.rs:170) is left to the caller (bytes that do not
 * form valid UTF-8 can only come from id sequences that split a character), e.g. Python's
 * bytes.decode("utf-8", "replace"), which substitutes the same maximal invalid subparts. */
#define TKAMD_SKIP_SPECIAL 1u
typedef struct tkamd_text tkamd_text;
int tkamd_decode_batch(tkamd_tokenizer* tok, const uint32_t* ids, const int64_t* tok_offsets, int64_t n_docs,
                       uint32_t flags, tkamd_text** out);
int64_t         tkamd_text_n_docs(const tkamd_text* b);
int64_t         tkamd_text_n_bytes(const tkamd_text* b);
const uint8_t*  tkamd_text_bytes(const tkamd_text* b);         /* [n_bytes]                    */
const int64_t*  tkamd_text_doc_offsets(const tkamd_text* b);   /* [n_docs+1] CSR into bytes    */
void            tkamd_text_free(tkamd_text* b);

/* ---- decode_batch, device entry: ids already resident in HBM, the text stays in HBM ------------------
 * For callers whose ids never were on the host -- a generation loop's padded [B, L] output tensor, rollouts decoded with one
 * tokenizer and encoded again with another -- and who want the text where tkamd_encode_batch_device reads it.
 *   in : d_ids[n_ids], uint32 (an int32 tensor's bit patterns are the same thing) or, with TKAMD_DECODE_IDS_I64, int64 (torch.long);
 *        sequence d is d_ids[d_begin[d] .. d_end[d]).  The ranges may come in any order, overlap, leave gaps or be empty: a packed CSR
 *        is d_begin = off, d_end = off + 1; row r of a right- or left-padded [B, L] tensor is begin = r * L + pad_left[r],
 *        end = begin + len[r].  n_ids bounds them: a range with begin > end, begin < 0 or end > n_ids is found ON THE DEVICE, copies
 *        nothing (it never causes a read outside d_ids) and fails the call with TKAMD_ERR_INVALID naming the first such sequence.
 *        An int64 value outside [0, 2^32) decodes to nothing, like any id without a token (-100 labels, -1 fillers).
 *   out: VALID UTF-8 -- for the ByteLevel decoder String::from_utf8_lossy (byte_level.rs:170) runs on the device, per sequence: every
 *        maximal invalid subpart becomes one U+FFFD; a sequence that ends in E2 82 gets one, and the next one, beginning with AC, one of
 *        its own (every other decoder emits token strings; ByteFallback writes its own U+FFFD) -- as one buffer + CSR with
 *        TKAMD_TEXT_PAD zero bytes behind it: exactly what tkamd_encode_batch_device takes.  flags: TKAMD_SKIP_SPECIAL as above.
 * Everything runs on `hip_stream` in the workspace keyed by that stream.  The call sizes its buffers from counts the device computes,
 * so it WAITS for the stream: twice (the token count of the ranges, with the range check; the byte count of the text), and a third
 * time for the ByteLevel decoder (the count of invalid subparts, with the size of the repaired text: a text without one keeps its
 * buffer and skips the repair).  The outputs stay in HBM and are valid until the next decode call on the same handle and stream; an
 * encode call on that handle does not move them.  The limits of the host entry hold (fewer than 2^31 tokens, less than 4 GiB of
 * text), unsupported decoders are refused with the same messages, a host-only handle gets TKAMD_ERR_DEVICE, a multi-device handle
 * decodes on devices[0]. */
#define TKAMD_DECODE_IDS_I64 2u            /* d_ids holds int64 (torch.long), else uint32 / int32 bit patterns */
typedef struct tkamd_device_text {
    const uint8_t* d_bytes;        /* [n_bytes] valid UTF-8, followed by >= TKAMD_TEXT_PAD zero bytes */
    const int64_t* d_doc_offsets;  /* [n_docs + 1] CSR into d_bytes                                   */
    const int64_t* d_n_bytes;      /* [1]                                                             */
    int64_t        n_bytes;        /* the same count, known when the call returns (-1: a fused stream step) */
} tkamd_device_text;
int tkamd_decode_batch_device(tkamd_tokenizer* tok, const void* d_ids, int64_t n_ids,
                              const int64_t* d_begin, const int64_t* d_end, int64_t n_docs,
                              uint32_t flags, void* hip_stream, tkamd_device_text* out);
/* A result of the call above copied to host memory on `hip_stream` (the call waits for it): bytes[0 .. text->n_bytes + n_slack) -- n_slack
 * <= TKAMD_TEXT_PAD bytes of the zero slack behind the text --, doc_offsets[0 .. n_docs] and *n_bytes, the count as the device holds it.
 * Any of the three may be NULL.  text->n_bytes < 0 (a fused stream step): the count is fetched first, one more wait.  For bindings that have no HIP runtime of their own to copy with; a consumer on the device reads the
 * pointers of tkamd_device_text directly. */
int tkamd_device_text_read(tkamd_tokenizer* tok, const tkamd_device_text* text, int64_t n_docs, int64_t n_slack, void* hip_stream,
                           uint8_t* bytes, int64_t* doc_offsets, int64_t* n_bytes);

/* ---- streaming decode: DecodeStream for a batch of running sequences, state and text in HBM ---------------
 * The reference's DecodeStream (tokenizer/mod.rs step_decode_stream; Python tokenizers.decoders.DecodeStream) is one object per
 * sequence, stepped on the host.  A tkamd_decode_stream holds n_streams of them for one tokenizer handle: a step takes ONE new id per
 * stream from HBM and leaves, per stream, the text that just became printable -- bit for bit what n_streams DecodeStreams return.
 * Per stream the device keeps a window of ids and two counts (the reference's ids, prefix -- always the decode of the first ids of
 * the window, so no text is stored -- and prefix_index); a step decodes three short ranges of every window with the range decode of
 * tkamd_decode_batch_device (so first- and last-token forms, CTC's dedup, ByteFallback's runs and the lossy UTF-8 repair apply to the
 * WINDOW, as in the reference), compares, emits and drains.
 *   new  : flags = TKAMD_SKIP_SPECIAL or 0, kept for every step, and TKAMD_STREAM_FUSED (below).  window = the most ids one stream's window may hold (0: 32; at least 2;
 *          the reference's grows without bound -- it holds the ids since the last chunk, 1 - 3 on ordinary text).  n_streams >= 0.
 *          A host-only handle gets TKAMD_ERR_DEVICE, a decoder outside the decode path TKAMD_ERR_UNSUPPORTED with decode_batch's message;
 *          a multi-device handle streams on devices[0].  The object must be freed before its tokenizer.
 *   reset: the streams which[0 .. n) (host indices; NULL: all of them) are empty again -- a slot of a continuous batch taken by a new
 *          sequence.  Enqueue only.
 *   seed : reset of ONE stream whose window then holds ids[0 .. n) (host ids): the reference constructor's ids=.  n > window is
 *          TKAMD_ERR_INVALID.  Enqueue only.
 *   step : d_ids[n_streams] in HBM, uint32 / int32 bit patterns or, with TKAMD_DECODE_IDS_I64, int64 (a value outside [0, 2^32) is an id
 *          without a token, as above); d_active uint8[n_streams] in HBM or NULL (all): a stream with 0 is not stepped, its state untouched.
 *          With TKAMD_STREAM_IDS_HOST both are HOST arrays, which the call copies down itself (bindings without a HIP runtime).
 *          *text: n_streams documents, document s = the chunk of stream s (empty for every status but 1), TKAMD_TEXT_PAD zero bytes
 *          behind the text.  *d_status: uint8[n_streams] in HBM --
 *            0 stepped, nothing to emit (the reference's None)     1 chunk     2 not stepped (inactive)
 *            3 InvalidPrefix: the step's string does not start with the prefix (the reference's error); the state is what the reference
 *              leaves -- the window holds the id, nothing is drained -- and the stream may be stepped again
 *            4 window full: the id did not fit.  The stream is stuck -- every later step of it reports 4 -- until it is reset.
 *          Text and status live in buffers of the stream object: valid until its next step, whatever else runs on the handle.
 *          The step WAITS for hip_stream as the range decode does (two times, three for the ByteLevel decoder) and once more for the
 *          byte count of the chunks (text->n_bytes).
 *   read : the last step's text (with n_slack <= TKAMD_TEXT_PAD bytes of its slack), its CSR [n_streams + 1] and its status [n_streams]
 *          copied to host memory in one wait; any of the three may be NULL.
 *   peek : (tests, debugging) the state of ONE stream on the host, after a wait for the whole device: up to cap ids of its window,
 *          their count *n, and the reference's prefix as ids (*pe: prefix = decode of the first *pe ids) and prefix_index (*pi).
 *   info : whether the object is fused (below), and what it allocated for that: the bytes its chunk buffer holds and its string scratch
 *          (both 0 for an object that is not fused, whose buffers follow the counts of each step).  Any pointer may be NULL.
 * One call at a time per object (calls are serialised inside); the caller orders its streams as for any stream-ordered API.
 *
 * A FUSED object (new with TKAMD_STREAM_FUSED) steps WITHOUT a host wait: push, the three strings of every window and the decision run in
 * one kernel with a lane per stream (over the very per-token device functions of the range decode), followed by the scan of the chunk
 * lengths, the copy and the zero slack -- 6 kernel launches, the same for every decoder and whatever the windows hold.  Everything a
 * step touches is allocated by `new`, sized by a bound instead of counts: a decoded window is at most window x max(L, 3) bytes, L = the
 * longest string one id decodes to in either position form (for ByteLevel: repaired by from_utf8_lossy on its own, which bounds what it
 * contributes in any company) and 3 = one U+FFFD per byte token of a run that is not UTF-8; 3 such strings a stream (4 for ByteLevel) and
 * a chunk buffer of n_streams x window x max(L, 3) bytes.  `new` fails with TKAMD_ERR_INVALID naming n_streams, window and L when strings
 * and chunks together exceed 1 GiB.  A step of a fused object only enqueues: no synchronisation, no copy to the host, no allocation; it
 * returns text->d_bytes / d_doc_offsets / d_n_bytes as above and text->n_bytes = -1 -- the host does not hold the count; it is
 * *text->d_n_bytes (and d_doc_offsets[n_streams]) once the stream has drained.  Status values and every state transition are those
 * of an object that is not fused.  Such a step can be captured into a HIP graph and replayed: step once outside the capture, keep d_ids
 * (and d_active) at fixed addresses and write the new ids there before each replay.  TKAMD_STREAM_IDS_HOST is allowed on a fused object
 * but stages through pinned host memory of the object and may wait for the previous staging: not a form to capture.  read,
 * tkamd_device_text_read and the Python helpers fetch the count from the device first when text->n_bytes < 0 (every time: a replayed graph
 * refills the buffers without a call); a bytes buffer handed to them must then hold the chunk capacity of `info` + n_slack, or be sized after
 * asking tkamd_device_text_read for *n_bytes alone.  reset, seed and peek work on both kinds of object (one state layout). */
#define TKAMD_STREAM_IDS_HOST 4u           /* tkamd_decode_stream_step: d_ids / d_active are host memory */
#define TKAMD_STREAM_FUSED 8u              /* tkamd_decode_stream_new: a step only enqueues (one fused kernel, buffers sized by bounds) */
typedef struct tkamd_decode_stream tkamd_decode_stream;
int  tkamd_decode_stream_new(tkamd_tokenizer* tok, int64_t n_streams, int32_t window, uint32_t flags, tkamd_decode_stream** out);
void tkamd_decode_stream_free(tkamd_decode_stream* s);
int  tkamd_decode_stream_reset(tkamd_decode_stream* s, const int64_t* which, int64_t n, void* hip_stream);
int  tkamd_decode_stream_seed(tkamd_decode_stream* s, int64_t which_one, const uint32_t* ids, int64_t n, void* hip_stream);
int  tkamd_decode_stream_step(tkamd_decode_stream* s, const void* d_ids, const uint8_t* d_active, uint32_t flags, void* hip_stream,
                              tkamd_device_text* text, const uint8_t** d_status);
int  tkamd_decode_stream_read(tkamd_decode_stream* s, int64_t n_slack, void* hip_stream, uint8_t* bytes, int64_t* doc_offsets, uint8_t* status);
int  tkamd_decode_stream_peek(tkamd_decode_stream* s, int64_t which_one, uint32_t* ids, int64_t cap, int64_t* n, int64_t* pe, int64_t* pi);
int  tkamd_decode_stream_info(tkamd_decode_stream* s, int64_t* fused, int64_t* chunk_capacity, int64_t* scratch_bytes);

/* String::from_utf8_lossy of ONE sequence -- bytes[0 .. n) -- by the host run of the very per-byte decision the kernels make
 * (csrc/utf8_lossy_core.hpp): out[0 .. *n_out).  Takes no handle and needs no device.  cap: what out holds; *n_out is set even when
 * it is too small (TKAMD_ERR_INVALID then). */
int tkamd_probe_utf8_lossy(const uint8_t* bytes, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out);
/* The byte string token `id` contributes (first_position != 0: as the first kept token of a sequence), straight from
 * the load-time decode tables; *flags = 0 ordinary, 1 special, 2 no token has this id.  Works on host-only handles. */
int tkamd_decode_token(const tkamd_tokenizer* tok, uint32_t id, int first_position, uint8_t* out, int32_t cap,
                       int32_t* len, int32_t* flags);

/* Host-side probes of the load-time tables -- the lookups the kernels perform, on the host copy (test hooks; work on
 * host-only handles).  Return 1 on a hit, 0 on a miss, < 0 on a bad argument.
 *   tkamd_probe_word : raw pre-token bytes -> token id (vocab.get of bpe/model.rs:559-567, wordlevel/mod.rs:162-178);
 *                      *flags bit 0 = WORD_DIRECT (byte-level BPE: the merges of these bytes yield exactly [id])
 *   tkamd_probe_merge: (left id, right id) -> (rank, new id)   (the `merges` map of bpe/model.rs:252-275)          */
int tkamd_probe_word(const tkamd_tokenizer* tok, const uint8_t* bytes, int32_t len, uint32_t* id, uint32_t* flags);
int tkamd_probe_merge(const tkamd_tokenizer* tok, uint32_t left, uint32_t right, uint32_t* rank, uint32_t* new_id);
/* One edge of the WordPiece byte trie (the longest-match walk of wordpiece/mod.rs:245-258 as a trie): (node, byte) ->
 * (child, id of the piece ending there or 0xFFFFFFFF); node 0 = word-initial pieces, 1 = continuation pieces. */
int tkamd_probe_trie(const tkamd_tokenizer* tok, uint32_t node, uint32_t byte, uint32_t* child, uint32_t* id);
/* Encoding::truncate (tokenizer/encoding.rs:307-395) of a sequence of n_tokens to max_len with `stride`, direction Right (left = 0) or
 * Left, straight from the function the epilogue kernels call (csrc/overflow_core.hpp): returns the number of encodings it leaves
 * (1 = nothing is cut; 0 = the reference's assert stride < max_len) and, for part < that number, its token range (part 0 = the
 * truncated encoding, 1.. = Encoding.overflowing in order). */
int tkamd_probe_truncation(uint64_t n_tokens, uint32_t max_len, uint32_t stride, int left, uint32_t part, uint64_t* start, uint64_t* count);
/* BertNormalizer::normalize (normalizers/bert.rs:92-138) of ONE code point from the host copy of the generated tables:
 * out[0..*n) (at most 12 code points; 0 = the char is removed), *refused = 1 for the characters NFD's canonical ordering could
 * move (they survive the Mn filter with a non-zero combining class): whether it does depends on their neighbours, see
 * tkamd_probe_bert_alone. */
int tkamd_probe_bert_norm(const tkamd_tokenizer* tok, uint32_t cp, uint32_t* out, int32_t* n, int32_t* refused);
/* The Precompiled normalizer (normalizers/precompiled.rs) of ONE piece -- text[0 .. n): a document, or what lies between two added-token
 * matches -- by the host run of the very core the kernels run (csrc/precompiled_core.hpp): out[0 .. *n_out) the normalized bytes,
 * src[k] the first byte of the source char that byte k is aligned to (the chars the reference loses at a piece's start included).
 * cap: what out and src hold; *n_out is set even when it is too small (TKAMD_ERR_INVALID then). */
int tkamd_probe_precompiled(const tkamd_tokenizer* tok, const uint8_t* text, int64_t n, uint8_t* out, uint32_t* src, int64_t cap, int64_t* n_out);
/* A chain of NFD / Lowercase / StripAccents (info.normalizer == 5) over ONE piece -- text[0 .. n) -- by the host run of what the kernels
 * read, the per-char expansions composed at load: out[0 .. *n_out) the normalized bytes, src[k] the first byte of the source char
 * that byte k is aligned to.  cap: what out and src hold; *n_out is set even when it is too small (TKAMD_ERR_INVALID then). */
int tkamd_probe_norm_chain(const tkamd_tokenizer* tok, const uint8_t* text, int64_t n, uint8_t* out, uint32_t* src, int64_t cap, int64_t* n_out);
/* NFKC (info.normalizer == 6) over ONE piece -- text[0 .. n) -- by the host run of the very core the kernels run, the K mode of
 * csrc/nfc_core.hpp: out[0 .. *n_out) the normalized bytes, src[k] the first byte of the source char that byte k is aligned to.  A run of
 * more than 48 combining characters is refused (TKAMD_ERR_UNSUPPORTED), as a batch that holds one is.  cap: what out and src hold; *n_out
 * is set even when it is too small (TKAMD_ERR_INVALID then). */
int tkamd_probe_nfkc(const tkamd_tokenizer* tok, const uint8_t* text, int64_t n, uint8_t* out, uint32_t* src, int64_t cap, int64_t* n_out);
/* BertNormalizer strip_accents on the character whose lead byte is text[pos] (text[0 .. n) = one piece handed to the normalizer: a
 * document, or what lies between two added-token matches): *reorder = 1 if it survives the Mn filter with a non-zero combining
 * class (NFD's canonical ordering could move it), *alone = 1 if it is alone in its run of non-starters -- nothing moves; 0: the
 * device puts that run into canonical order (csrc/bert_norm_core.hpp bn_fix_run).  The very function the kernels call, on the host
 * copy of the tables. */
int tkamd_probe_bert_alone(const tkamd_tokenizer* tok, const uint8_t* text, int64_t n, int64_t pos, int32_t* reorder, int32_t* alone);
/* The NFD form of one code point as bn_fix_run sees it, from the host copy of the tables: *packed = n | per piece q, at bit 3 + 7q,
 * (rank of its canonical combining class among the classes in use, 0 = starter) | (survives the Mn filter) << 6; 0: no piece of
 * the form is a non-starter.  *flags = the per-character table flags (1 dropped by clean_text, 2 whitespace, 4 CJK, 8 reorderable,
 * 16 / 32 has an NFD / lowercase expansion, 64 / 128 first / last piece is a non-starter). */
int tkamd_probe_bert_nfd(const tkamd_tokenizer* tok, uint32_t cp, uint32_t* packed, uint32_t* flags);
/* Class flags of one code point from the host copy of the generated Unicode table: bit 0 \p{L}, 1 \p{N}, 2 \s (as
 * Oniguruma sees them, byte_level.rs:43-46), 3 \w, 4 \s (regex crate, whitespace.rs:22), 5 char::is_whitespace, 6 is_bert_punc. */
int tkamd_probe_unicode_flags(const tkamd_tokenizer* tok, uint32_t cp, uint32_t* flags);

/* Tokenizer.encode_special_tokens (tokenizer/mod.rs:752-759, AddedVocabulary::set_encode_special_tokens added_vocabulary.rs:249-255):
 * value != 0 -> the special tokens of the added vocabulary are no longer extracted from the text (find_matches skips them,
 * added_vocabulary.rs:450-453): their characters go through the normalizer, pre-tokenizer and model like any text.  Applies to the
 * batches enqueued after the call.  Off by default. */
int tkamd_encode_special_tokens(tkamd_tokenizer* tok, int value);

/* ---- word cache --------------------------------------------------------------------------------
 * What BPE::tokenize_with_cache keeps per thread (models/bpe/model.rs:573-586, utils/cache.rs): pre-token bytes -> its tokens.
 * `enable` != 0: every workspace of the handle keeps a table (1 M entries, in HBM) of the <= 16-byte words its batches have merged
 * (results of <= 4 tokens); later ids-only batches (TKAMD_OFFSETS_NONE) look such a word up instead of merging it again.  Like the
 * reference's cache it only fills, never evicts, and never changes a result.  `clear` != 0: forget everything (every workspace
 * zeroes its table before its next batch).  Off by default -- the default is the cache's counterpart WITHIN a batch, which keeps no
 * state: the first occurrence of a word the static tables do not settle goes to the model kernel, its other occurrences in the same
 * batch share the result (in-batch claims, csrc/kernels/lookup.hip; with or without offsets).  Switching this cache on replaces them.
 * A batch that shared nothing (more than 35 % of its pre-tokens still queued) pauses the claims for the handle's next 32 batches
 * : on text that never repeats a word they only cost. */
int tkamd_word_cache(tkamd_tokenizer* tok, int enable, int clear);

/* ---- the hot-word table learns the handle's text ---------------------------------------------
 * The lookup kernel keeps 960 settled words of <= 12 bytes in LDS (csrc/tables.hpp); a pre-token that is one of them costs no memory
 * round trip.  At load these are the lowest ids.  The handle's first batch of >= 8 MiB of text, and every 1024th such batch after it,
 * also counts which words stand as whole pre-tokens in a 1 MiB sample of it (k_hot_census, csrc/kernels/lookup.hip); the call that
 * synchronises that batch (tkamd_device_sync, or any host entry) reads the counts, and if the table they select would have settled two
 * points more of the sample it replaces the one in use, for every later batch of the handle on any stream.  Results never depend on
 * what the table holds.  A caller that never synchronises through the library keeps the load-time table; so does a multi-device handle.
 * `enable` == 0 stops the censuses (the table in use stays); the environment variable TKAMD_HOT_ADAPT=0, read when a handle is made,
 * does the same from the start.  At most seven tables replace the load-time one in a handle's life (old ones are kept until it is
 * freed: a launch enqueued on another stream may still read one); after that it keeps what it has. */
int tkamd_hot_adapt(tkamd_tokenizer* tok, int enable);
/* Diagnostics: the table in use (`blob`, up to blob_cap bytes: 1024 16-byte slots {key bytes 0..11, id | len << 24}, then 256 16-bit
 * displacements), the ids of the words that may ever stand in it (`eligible_ids`, up to ids_cap; *n_eligible: how many there are), and
 * stats[8] = {rebuilds so far, words in the table, pre-tokens the last census sampled, 1/10000ths of them the table then in use settles,
 * ... the table its counts selected, the tables' hash seed, 1 if the handle adapts, slots}.  Any pointer may be null.  Returns the
 * table's size in bytes (0 on a host-only handle). */
int tkamd_hot_table_read(tkamd_tokenizer* tok, void* blob, int64_t blob_cap, uint32_t* eligible_ids, int64_t ids_cap, int64_t* n_eligible, uint32_t* stats);
/* ... and what the last census counted: counts[i] = sampled pre-tokens that were the word eligible_ids[i].  Returns how many counts
 * there are (0 before the first census was read). */
int64_t tkamd_hot_census_counts(tkamd_tokenizer* tok, uint32_t* counts, int64_t cap);

/* ---- measurement hooks (bench.py roofline leg; not part of the reference surface) -----------
 * With profiling on, every kernel launch of the next device/host encode calls is bracketed by
 * HIP events on the launch stream.  tkamd_profile_read returns, per kernel, the accumulated
 * milliseconds and launch count since the last reset. */
#define TKAMD_MAX_STAGES 24
typedef struct tkamd_stage_time {
    char    name[48];
    double  ms_total;
    int64_t launches;
} tkamd_stage_time;
int tkamd_profile_enable(tkamd_tokenizer* tok, int on);
int tkamd_profile_read(tkamd_tokenizer* tok, tkamd_stage_time* stages, int max_stages, int* n_stages, int reset);

/* Work-queue sizes of the last synchronised batch: out[0] = pre-tokens sent to the 16-lane merge
 * kernel, out[1] = to the 64-lane kernel, out[2] = to the workgroup (long) kernel.  Behind the batch's counters and the handle's
 * adaptive settings (out[13..17]), the shape of the load-time tables, filled from the handle also before its first batch:
 * out[18] = slots of the short-word table, out[19] = its displacement buckets, out[20] = its largest displacement,
 * out[21] = slots of the merge table (out[18..20] are 0 on a host-only handle).  out[22] = the grid of the last batch's launch that
 * merges both LDS queues side by side (0: the batch ran none).  out[23..27]: the hot-word table -- rebuilds so far, words in it, and
 * of the last census the sampled pre-tokens and the 1/10000ths of them the table then in use / the table selected settle. */
int tkamd_profile_counters(tkamd_tokenizer* tok, uint32_t* out, int n);

/* Where the two longest kernels spend their time.  With the test hook TKAMD_PHASES (TKAMD_TEST_HOOKS=1 TKAMD_PHASES=1) the whole-word
 * lookup (which = 0) and the token compaction (which = 1) run as diagnostic instantiations that stamp the shader clock behind the
 * barriers that end their phases; out[0..7] = ticks summed over all workgroups and batches since the last reset
 * (lookup: 0 staging a tile, 1 expanding the mask bits, 2 pass 1 (LDS hot table), 3 pass 2 (perfect hash), 4 pass 3 (claims) +
 * waiting for the slowest wavefront; compaction: 0 loads + scan + publish, 1 LDS scatter, 2 look-back wait, 3 copy-out; 7 = the
 * whole kernel, both).  All zero without the variable.  A development aid: never set it in a measured run. */
int tkamd_debug_phases(tkamd_tokenizer* tok, int which, uint64_t* out, int reset);

/* Library version string, e.g. "tokenizers_amd 0.1.0 (gfx950)". */
const char* tkamd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TOKENIZERS_AMD_H */
