"""Checks of the densely packed load-time tables, shared by tests/test_dense_tables.py (the emulation build, no GPU) and
tests/test_dense_tables_gpu.py (-m gpu): the short-word table behind 16-bit displacements (capi/tables.cpp build_shortw_table) and the
merge table next to it, whose slots the same counters report (a dense sizing of it was measured and not kept, HISTORY.md).  What the
tables hold is checked through the product: a word the table holds comes back as its id without touching a merge queue, a word it
does not hold as the unk id; how they are packed is read from Tokenizer.queue_sizes() (tkamd_profile_counters, slots 18..21)."""
import ctypes as C
import json
import re

import numpy as np

ALPHA = "abcdefghijklmnopqrstuvwxyz0123456789_"
UNK = "<unk>"
WORD_DIRECT = 1
SHAPE_KEYS = ("shortw_slots", "shortw_buckets", "shortw_max_disp", "merge_slots")


def _word(rng, n):
    return "".join(ALPHA[i] for i in rng.integers(0, len(ALPHA), size=n))


def make_wordlevel(n_words: int, seed: int = 11):
    """n_words distinct words over [a-z0-9_], 1..16 bytes with every length present, 200 pairs of them equal in bytes 0..11 and different
    only in bytes 12..15 (the k3 array of the short-word table tells them apart), ids shuffled; the unk token on top.
    Returns (tokenizer.json, {word: id}, unk id, the pairs)."""
    rng = np.random.default_rng(seed)
    words, pairs = set(), []
    while len(pairs) < 200:
        n = int(rng.integers(13, 17))
        head, a, b = _word(rng, 12), _word(rng, n - 12), _word(rng, n - 12)
        if a != b and head + a not in words and head + b not in words:
            words.update((head + a, head + b))
            pairs.append((head + a, head + b))
    for n in range(1, 17):                                # every length is there ...
        while not any(len(w) == n for w in words):
            words.add(_word(rng, n))
    while len(words) < n_words:                           # ... and the rest is of any
        words.add(_word(rng, int(rng.integers(1, 17))))
    words = sorted(words)
    ids = rng.permutation(len(words) + 1)
    vocab = {w: int(ids[k]) for k, w in enumerate(words)}
    vocab[UNK] = int(ids[len(words)])
    js = json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": None,
                     "pre_tokenizer": {"type": "Whitespace"}, "post_processor": None, "decoder": None,
                     "model": {"type": "WordLevel", "vocab": vocab, "unk_token": UNK}})
    del vocab[UNK]
    return js, vocab, int(ids[len(words)]), pairs


def strangers(vocab: dict, n: int = 2000, seed: int = 12):
    """n words the vocabulary does not hold: half of them a vocabulary word with one of its bytes 12..15 changed, half of them random."""
    rng = np.random.default_rng(seed)
    long_words = sorted(w for w in vocab if len(w) >= 13)
    out = set()
    while len(out) < n // 2:
        w = long_words[int(rng.integers(0, len(long_words)))]
        k = int(rng.integers(12, len(w)))
        v = w[:k] + ALPHA[int(rng.integers(0, len(ALPHA)))] + w[k + 1:]
        if v not in vocab:
            out.add(v)
    while len(out) < n:
        v = _word(rng, int(rng.integers(1, 17)))
        if v not in vocab:
            out.add(v)
    return sorted(out)


def check_wordlevel(n_words: int, want_slots: int):
    import tokenizers_amd as ta
    js, vocab, unk_id, pairs = make_wordlevel(n_words)
    assert len(vocab) == n_words and {len(w) for w in vocab} == set(range(1, 17))
    assert all(a[:12] == b[:12] and a[12:] != b[12:] and a in vocab and b in vocab for a, b in pairs)
    tok = ta.Tokenizer.from_str(js, device=0)
    shape = tok.queue_sizes()                              # (before the first batch: the shape comes from the handle)
    assert shape["shortw_slots"] == want_slots, shape
    assert shape["shortw_max_disp"] > 255, shape           # the 16-bit path really ran
    assert 0 < shape["shortw_buckets"] <= max(16, n_words // 2), shape
    words = list(vocab)
    want = np.array([vocab[w] for w in words], dtype=np.uint32)
    # every word a document of its own
    got = tok.encode_batch_fast(words, add_special_tokens=False)
    assert np.array_equal(np.asarray(got.tok_offsets), np.arange(len(words) + 1)), "a word did not come back as one token"
    bad = np.flatnonzero(np.asarray(got.ids).view(np.uint32) != want)
    assert bad.size == 0, (bad.size, words[int(bad[0])])
    q = tok.queue_sizes()
    assert q["merge16"] == 0, q
    assert {k: q[k] for k in SHAPE_KEYS} == {k: shape[k] for k in SHAPE_KEYS}
    # all of them in one document
    got = tok.encode_batch_fast([" ".join(words)], add_special_tokens=False)
    assert np.array_equal(np.asarray(got.ids).view(np.uint32), want)
    assert tok.queue_sizes()["merge16"] == 0
    # words it does not hold
    out = strangers(vocab)
    assert len(out) == 2000
    got = tok.encode_batch_fast(out + [" ".join(out)], add_special_tokens=False)
    ids = np.asarray(got.ids).view(np.uint32)
    assert ids.size == 4000 and (ids == unk_id).all(), out[int(np.flatnonzero(ids != unk_id)[0]) % 2000]
    assert tok.queue_sizes()["merge16"] == 0
    return js, shape


def check_determinism(js: str, first: dict):
    import tokenizers_amd as ta
    again = ta.Tokenizer.from_str(js, device=0).queue_sizes()
    assert {k: again[k] for k in SHAPE_KEYS} == {k: first[k] for k in SHAPE_KEYS}


def check_c2(js: str):
    """The flagship tokenizer (GPT-2 byte-level BPE, 50 k entries): every vocabulary entry of <= 16 bytes that the load-time proof
    flagged WORD_DIRECT and that is one pre-token by itself comes back as its id straight from the tables; the short-word table is packed
    into 65,536 slots; the merge table holds every merge and nothing else."""
    import tokenizers_amd as ta
    from oracle.decode_oracle import CHAR_BYTES
    tok = ta.Tokenizer.from_str(js, device=0)
    lib, h = tok._lib, tok._h
    shape = tok.queue_sizes()
    assert shape["shortw_slots"] == 65536, shape
    assert shape["merge_slots"] >= len(json.loads(js)["model"]["merges"]), shape      # (reported; its sizing is host_model.cpp build_merge_table's)
    d = json.loads(js)
    vocab = d["model"]["vocab"]
    one_pretoken = re.compile(rb" ?[A-Za-z]+| ?[0-9]+")
    idv, fl = C.c_uint32(0), C.c_uint32(0)
    docs, want = [], []
    for t, i in vocab.items():
        try:
            raw = bytes(CHAR_BYTES[c] for c in t)
        except KeyError:
            continue
        if not raw or len(raw) > 16 or not one_pretoken.fullmatch(raw):
            continue
        if lib.tkamd_probe_word(h, raw, len(raw), C.byref(idv), C.byref(fl)) == 1 and (fl.value & WORD_DIRECT):
            assert idv.value == i, t
            docs.append(raw.decode("ascii"))
            want.append(i)
    assert len(docs) > 10000, len(docs)
    got = tok.encode_batch_fast(docs, add_special_tokens=False)
    assert np.array_equal(np.asarray(got.tok_offsets), np.arange(len(docs) + 1)), "a direct word did not come back as one token"
    bad = np.flatnonzero(np.asarray(got.ids).view(np.uint32) != np.array(want, dtype=np.uint32))
    assert bad.size == 0, (bad.size, docs[int(bad[0])])
    q = tok.queue_sizes()
    assert (q["merge16"], q["merge32"], q["merge64"], q["merge_long"], q["merge_huge"]) == (0, 0, 0, 0, 0), q
    # the merge table: every merge of the file, and a thousand pairs that are no merges
    rk, nid = C.c_uint32(0), C.c_uint32(0)
    last = {}
    for r, m in enumerate(d["model"]["merges"]):
        a, b = m if isinstance(m, list) else m.split(" ")
        last[(vocab[a], vocab[b])] = (r, vocab[a + b])                   # (duplicate pairs: the last rank wins)
    for (a, b), (r, n) in last.items():
        assert lib.tkamd_probe_merge(h, a, b, C.byref(rk), C.byref(nid)) == 1, (a, b)
        assert (rk.value, nid.value) == (r, n), (a, b)
    rng = np.random.default_rng(13)
    n_none = 0
    while n_none < 1000:
        a, b = (int(x) for x in rng.integers(0, len(vocab), size=2))
        if (a, b) in last:
            continue
        assert lib.tkamd_probe_merge(h, a, b, C.byref(rk), C.byref(nid)) == 0, (a, b)
        n_none += 1
    return shape
