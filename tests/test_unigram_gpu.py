"""Unigram on the device: the Viterbi kernel (kernels/unigram.hip) behind the "▁" front against the reference wheel's vectors
(tools/make_golden_unigram.py) -- every field, through every entry -- and a live differential where the wheel is importable."""
import json
import random

import numpy as np
import pytest

import tokenizers_amd as ta
from tests.helpers import N, char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAMES = ["unigram_ms", "unigram_ms_nobytes", "unigram_adv"]
MS = "▁"


def _tok(name, **kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(name), device=0, **kw)


def _csr(b, i):
    return int(b.tok_offsets[i]), int(b.tok_offsets[i + 1])


def _byte_offsets(doc, coffs):
    m = char_to_byte(doc)
    return [[m[a], m[b]] for a, b in coffs]


@pytest.mark.parametrize("name", NAMES)
def test_vectors_encode_batch(name):
    v = load_vectors(name)
    got = _tok(name).encode_batch(v["docs"], add_special_tokens=False)
    for i, d in enumerate(v["docs"]):
        e = got[i]
        assert list(e.ids) == v["ids"][i], (name, d)
        assert [list(o) for o in e.offsets] == v["offsets_char"][i], (name, d)
        assert list(e.word_ids) == v["words"][i], (name, d)


@pytest.mark.parametrize("name", NAMES)
def test_vectors_csr_byte_offsets_fast_and_packed(name):
    v = load_vectors(name)
    tok = _tok(name)
    b = tok.encode_batch_csr(v["docs"], offsets="byte", word_ids=True)
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    buf, off = ta.pack_documents(v["docs"])
    p = tok.encode_packed(buf, off)
    for i, d in enumerate(v["docs"]):
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i], (name, d)
        assert b.offsets[a:z].tolist() == _byte_offsets(d, v["offsets_char"][i]), (name, d)
        assert b.word_ids[a:z].tolist() == v["words"][i], (name, d)
        assert list(fast[i].ids) == v["ids"][i], (name, d)
        a, z = _csr(p, i)
        assert p.ids[a:z].tolist() == v["ids"][i], (name, d)


def test_known_answers():
    tok = _tok("unigram_adv")
    e = tok.encode_batch(["ab", "e ee", "xy", "xx<unk>", "a<s>b"], add_special_tokens=False)
    assert list(e[0].tokens) == [MS, "ab"]                              # a tie: the earliest start wins (the prepended "▁" is the first word's)
    dup = [i for i, (p, _) in enumerate(json.loads(load_tokenizer_json("unigram_adv"))["model"]["vocab"]) if p == "e"]
    assert len(dup) == 2 and list(e[1].ids) == [0, dup[1], 0, dup[1], dup[1]]      # the duplicated piece: the later id, and with its score e + e beats ee
    assert list(e[2].tokens) == [MS, "xy"]                              # two unks outscore the piece, and the fused run is the piece
    assert list(e[3].ids) == [0, 4] and [tuple(o) for o in e[3].offsets] == [(0, 1), (0, 7)]      # unknown chars and the literal unk piece behind them: ONE token
    assert list(e[4].tokens) == [MS + "a", "<s>", "b"] and [tuple(o) for o in e[4].offsets] == [(0, 1), (1, 4), (4, 5)]      # ▁a ties with ▁ + a: met first
    tok = _tok("unigram_ms")
    e = tok.encode_batch(["aꙮ🦀b"], add_special_tokens=False)[0]
    runs = [tuple(o) for o, t in zip(e.offsets, e.tokens) if t.startswith("<0x")]
    assert runs == [(1, 3)] * 7                                         # every byte token carries the offsets of the whole run (3 + 4 bytes, two chars)


def _special_docs(v):
    docs = [d for d in v["docs"] if "<s>" in d or "</s>" in d or "<unk>" in d or "<x>" in d]
    assert docs
    return docs, [v["docs"].index(d) for d in docs]


@pytest.mark.parametrize("name", NAMES)
def test_special_tokens_in_text(name):
    """added tokens in the text: by speculation (the batch is run again once the detection pass saw one), then without it."""
    v = load_vectors(name)
    docs, idx = _special_docs(v)
    tok = _tok(name)
    for _ in range(2):
        got = tok.encode_batch(docs, add_special_tokens=False)
        for k, i in enumerate(idx):
            assert list(got[k].ids) == v["ids"][i]
            assert [list(o) for o in got[k].offsets] == v["offsets_char"][i]
            assert list(got[k].word_ids) == v["words"][i]


@pytest.mark.parametrize("name", NAMES)
def test_encode_special_tokens(name, ref_tokenizers):
    docs, _ = _special_docs(load_vectors(name))
    tok = _tok(name)
    w = ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name))
    w.encode_special_tokens = True
    tok.encode_special_tokens = True
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    for k in range(len(docs)):
        assert list(got[k].ids) == exp[k].ids, docs[k]
        assert [tuple(o) for o in got[k].offsets] == exp[k].offsets, docs[k]


@pytest.mark.parametrize("name", NAMES)
def test_template_pairs_truncation_padding(name):
    v = load_vectors(name)
    tok = _tok(name)
    got = tok.encode_batch(v["docs"], add_special_tokens=True)
    for i in range(len(v["docs"])):
        assert list(got[i].ids) == v["special"]["ids"][i]
        assert [list(o) for o in got[i].offsets] == v["special"]["offsets_char"][i]
        assert list(got[i].word_ids) == v["special"]["words"][i]
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    for i in range(len(pairs)):
        assert list(got[i].ids) == v["pairs"]["ids"][i], pairs[i]
        assert list(got[i].type_ids) == v["pairs"]["type_ids"][i]
        assert [list(o) for o in got[i].offsets] == v["pairs"]["offsets_char"][i]
        assert list(got[i].word_ids) == v["pairs"]["words"][i]
    single = v["trunc"]["inputs"]
    tt = _tok(name)
    tt.enable_truncation(max_length=v["trunc"]["max_length"], stride=v["trunc"]["stride"])
    got = tt.encode_batch_csr(single, add_special_tokens=True, overflowing=True)
    for i in range(len(single)):
        e = got[i]
        assert list(e.ids) == v["trunc"]["ids"][i]
        assert [list(o.ids) for o in e.overflowing] == v["trunc"]["overflowing"][i]
    tp = _tok(name)
    tp.enable_padding(pad_id=0, pad_token=v["pad"]["pad_token"])
    got = tp.encode_batch(single, add_special_tokens=True)
    for i in range(len(single)):
        assert list(got[i].ids) == v["pad"]["ids"][i]
        assert list(got[i].attention_mask) == v["pad"]["attention_mask"][i]


@pytest.mark.parametrize("name", NAMES)
def test_mixed_batch_and_pretokenized(name):
    v = load_vectors(name)
    tok = _tok(name)
    pairs = [tuple(p) for p in v["pairs"]["inputs"][:40]]
    singles = [p[0] for p in pairs]
    exp_single = {d: v["special"]["ids"][i] for i, d in enumerate(v["docs"])}
    items, exp = [], []
    for i in range(40):
        items.append(singles[i]); exp.append(exp_single[singles[i]])
        items.append(pairs[i]); exp.append(v["pairs"]["ids"][i])
    got = tok.encode_batch(items, add_special_tokens=True)
    for i in range(len(items)):
        assert list(got[i].ids) == exp[i], items[i]
    got = tok.encode_batch(v["pretok"]["inputs"], is_pretokenized=True, add_special_tokens=False)
    for i in range(len(v["pretok"]["inputs"])):
        assert list(got[i].ids) == v["pretok"]["ids"][i]
        assert list(got[i].word_ids) == v["pretok"]["words"][i]
        assert [list(o) for o in got[i].offsets] == v["pretok"]["offsets_char"][i]


@pytest.mark.needs_hw
def test_device_entry():
    import torch
    v = load_vectors("unigram_ms")
    tok = _tok("unigram_ms")
    buf, off = ta.pack_documents(v["docs"])
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(v["docs"]), int(off[-1]), stream=torch.cuda.current_stream().cuda_stream).sync()
    ids = b.ids_tensor().cpu().numpy().view("uint32")
    tof = b.tok_offsets_tensor().cpu().numpy()
    for i in range(len(v["docs"])):
        assert ids[tof[i]:tof[i + 1]].tolist() == v["ids"][i]


def test_same_device_twice():
    v = load_vectors("unigram_ms")
    tok = _tok("unigram_ms")
    two = ta.Tokenizer.from_str(load_tokenizer_json("unigram_ms"), device=[0, 0])
    docs = v["docs"] * 3
    a = tok.encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)


@pytest.mark.parametrize("name", NAMES)
def test_decode_round_trip(name):
    """the decode tables come from the array vocabulary, per index (unigram_ms*: Sequence[Replace, ByteFallback, Fuse, Strip]; unigram_adv: none)"""
    v = load_vectors(name)
    tok = _tok(name)
    assert tok.decode_batch(v["ids"], skip_special_tokens=False) == v["decoded"]
    got = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert tok.decode_batch([list(got[i].ids) for i in range(len(v["docs"]))], skip_special_tokens=False) == v["decoded"]
    if name == "unigram_adv":                                           # both ids of the duplicated piece decode to it
        dup = [i for i, (p, _) in enumerate(json.loads(load_tokenizer_json(name))["model"]["vocab"]) if p == "e"]
        assert tok.decode_batch([[dup[0]], [dup[1]]], skip_special_tokens=False) == ["e", "e"]


@pytest.mark.parametrize("name", NAMES)
def test_pretokens_beyond_8kb_and_repeated_words(name):
    """pre-tokens of 8,192 / 8,193 bytes and about 20 KB (the state in HBM, at the word's own bytes), one word thousands of times (claims)"""
    v = load_vectors(name)
    from tests.unigram_cases import long_docs
    docs, exp = long_docs(), v["long"]
    tok = _tok(name)
    got = tok.encode_batch(docs, add_special_tokens=False)
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    for k, d in enumerate(docs):
        offs = [tuple(exp["offsets_char"][k][2 * j:2 * j + 2]) for j in range(len(exp["ids"][k]))]
        assert list(got[k].ids) == exp["ids"][k], (name, k)
        assert [tuple(o) for o in got[k].offsets] == offs, (name, k)
        assert list(got[k].word_ids) == exp["words"][k], (name, k)
        m = char_to_byte(d)
        a, z = _csr(b, k)
        assert b.ids[a:z].tolist() == exp["ids"][k], (name, k)
        assert b.offsets[a:z].tolist() == [[m[x], m[y]] for x, y in offs], (name, k)


def test_unk_id_null_fails_the_call_and_the_handle_stays_usable():
    d = json.loads(load_tokenizer_json("unigram_adv"))
    d["model"]["unk_id"] = None
    tok = ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=0)
    ok = tok.encode_batch(["ab abc", "hello"], add_special_tokens=False)
    assert list(ok[0].tokens) == [MS, "ab", MS, "abc"]
    with pytest.raises(ta.TokenizersAmdError, match="MissingUnkToken"):      # (ERR_MISSING_UNK, as WordLevel without its unk_token)
        tok.encode_batch(["ab", "a ꙮ b"], add_special_tokens=False)
    again = tok.encode_batch(["ab abc", "hello"], add_special_tokens=False)
    assert [list(e.ids) for e in again] == [list(e.ids) for e in ok]


def _random_docs(rng, n):
    pool = ["a", "b", "ab", "c", "d", "e", "xy", "x", "the", "ing", " ", "  ", "\t", "\n", MS, "<s>", "</s>", "<unk>", "<x>", "中", "文字", "😀", "ꙮ", "é", "ß", "Hello", "world", ",", ".",
            "12", "ё", "ﬁ", "​", "hello", "q" * 17, "w" * 30]
    return ["".join(rng.choice(pool) for _ in range(rng.randint(0, 30))) for _ in range(n)]


@pytest.mark.parametrize("name", NAMES)
def test_live_differential(name, ref_tokenizers):
    w = ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name))
    tok = _tok(name)
    from oracle import synth
    rng = random.Random(301 + NAMES.index(name))
    docs = _random_docs(rng, N(3000)) + synth.gen_lines(N(1000), text_seed=79)
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    for k, d in enumerate(docs):
        assert list(got[k].ids) == exp[k].ids, d
        assert [tuple(o) for o in got[k].offsets] == exp[k].offsets, d
        assert list(got[k].word_ids) == exp[k].word_ids, d
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    for k, d in enumerate(docs):
        m = char_to_byte(d)
        a, z = _csr(b, k)
        assert b.offsets[a:z].tolist() == [[m[x], m[y]] for x, y in exp[k].offsets], d
