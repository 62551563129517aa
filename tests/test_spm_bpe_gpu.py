"""SentencePiece-style BPE on the device: the "▁" front (kernels/metaspace.hip) in its three layouts against the reference wheel's
vectors (tools/make_golden_spm_bpe.py) -- every field, through every entry -- and a live differential where the wheel is importable."""
import random

import numpy as np
import pytest

import tokenizers_amd as ta
from tests.helpers import N, char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAMES = ["spm_bpe_llama2", "spm_bpe_first", "spm_bpe_split", "spm_bpe_replace_only"]
MS = "▁"
NONE32 = 0xFFFFFFFF


def _tok(name, **kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(name), device=0, **kw)


def _csr(b, i):
    a, z = int(b.tok_offsets[i]), int(b.tok_offsets[i + 1])
    return a, z


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
def test_vectors_csr_byte_offsets_and_fast(name):
    v = load_vectors(name)
    tok = _tok(name)
    b = tok.encode_batch_csr(v["docs"], offsets="byte", word_ids=True)
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    for i, d in enumerate(v["docs"]):
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i], (name, d)
        assert b.offsets[a:z].tolist() == v["offsets"][i], (name, d)
        assert b.word_ids[a:z].tolist() == v["words"][i], (name, d)
        assert list(fast[i].ids) == v["ids"][i], (name, d)


@pytest.mark.parametrize("name", NAMES)
def test_known_answers(name):
    tok = _tok(name)
    e = tok.encode_batch(["a<s>b c"], add_special_tokens=False)[0]
    exp_tokens = {"spm_bpe_first": ["▁a", "<s>", "b", "▁c"], "spm_bpe_replace_only": ["a", "<s>", "b", "▁c"]}.get(name, ["▁a", "<s>", "▁b", "▁c"])
    assert list(e.tokens) == exp_tokens
    assert [tuple(o) for o in e.offsets] == [(0, 1), (1, 4), (4, 5), (5, 7)]
    assert list(e.word_ids) == ([0, 1, 2, 3] if name == "spm_bpe_split" else [0, 1, 2, 2])
    if name == "spm_bpe_llama2":
        e = tok.encode_batch(["Hello world", "  two  spaces "], add_special_tokens=False)
        assert list(e[0].tokens) == ["▁He", "ll", "o", "▁w", "or", "l", "d"]
        assert [tuple(o) for o in e[1].offsets][:3] == [(0, 1), (0, 1), (1, 3)]


def _special_docs(v):
    docs = [d for d in v["docs"] if "<s>" in d or "</s>" in d or "<unk>" in d]
    assert docs
    return docs, [v["docs"].index(d) for d in docs]


@pytest.mark.parametrize("name", NAMES)
def test_special_tokens_in_text(name):
    """<s> / </s> in the text: by speculation (the batch is run again once the detection pass saw one), then without it."""
    v = load_vectors(name)
    docs, idx = _special_docs(v)
    tok = _tok(name)
    for _ in range(2):                                  # (the first batch speculates, the next ones run the matching passes)
        got = tok.encode_batch(docs, add_special_tokens=False)
        for k, i in enumerate(idx):
            assert list(got[k].ids) == v["ids"][i]
            assert list(got[k].word_ids) == v["words"][i]


@pytest.mark.parametrize("name", NAMES)
def test_encode_special_tokens(name, ref_tokenizers):
    """encode_special_tokens=True: the added tokens are matched as text."""
    docs, _ = _special_docs(load_vectors(name))
    tok = _tok(name)
    w = ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name))
    w.encode_special_tokens = True
    tok.encode_special_tokens = True
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    for k in range(len(docs)):
        assert list(got[k].ids) == exp[k].ids
        assert [tuple(o) for o in got[k].offsets] == exp[k].offsets


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
    single = v["docs"][:len(v["trunc"]["ids"])]
    tt = _tok(name)
    tt.enable_truncation(max_length=v["trunc"]["max_length"], stride=v["trunc"]["stride"])
    got = tt.encode_batch_csr(single, add_special_tokens=True, overflowing=True)
    for i in range(len(single)):
        e = got[i]
        assert list(e.ids) == v["trunc"]["ids"][i]
        assert [list(o.ids) for o in e.overflowing] == v["trunc"]["overflowing"][i]
    tp = _tok(name)
    tp.enable_padding(pad_id=0, pad_token="<unk>")
    got = tp.encode_batch(single, add_special_tokens=True)
    for i in range(len(single)):
        assert list(got[i].ids) == v["pad"]["ids"][i]
        assert list(got[i].attention_mask) == v["pad"]["attention_mask"][i]


@pytest.mark.parametrize("name", NAMES)
def test_mixed_batch(name):
    v = load_vectors(name)
    tok = _tok(name)
    pairs = [tuple(p) for p in v["pairs"]["inputs"][:40]]
    items, exp = [], []
    for i in range(40):
        items.append(v["docs"][i]); exp.append(v["special"]["ids"][i])
        items.append(pairs[i]); exp.append(v["pairs"]["ids"][i])
    got = tok.encode_batch(items, add_special_tokens=True)
    for i in range(len(items)):
        assert list(got[i].ids) == exp[i], items[i]


@pytest.mark.parametrize("name", NAMES)
def test_pretokenized(name):
    v = load_vectors(name)
    tok = _tok(name)
    got = tok.encode_batch(v["pretok"]["inputs"], is_pretokenized=True, add_special_tokens=False)
    for i in range(len(v["pretok"]["inputs"])):
        assert list(got[i].ids) == v["pretok"]["ids"][i]
        assert list(got[i].word_ids) == v["pretok"]["words"][i]
        assert [list(o) for o in got[i].offsets] == v["pretok"]["offsets_char"][i]
    e = tok.encode_batch([["ab", "cd ef"]], is_pretokenized=True, add_special_tokens=False)[0]
    if name != "spm_bpe_replace_only":
        assert "".join(e.tokens).startswith(MS + "a") and (MS + "c") in "".join(e.tokens)


@pytest.mark.parametrize("name", NAMES)
def test_packed_and_device_entries(name):
    v = load_vectors(name)
    tok = _tok(name)
    buf, off = ta.pack_documents(v["docs"])
    b = tok.encode_packed(buf, off)
    for i in range(len(v["docs"])):
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i]


@pytest.mark.needs_hw
def test_device_entry():
    import torch
    v = load_vectors("spm_bpe_llama2")
    tok = _tok("spm_bpe_llama2")
    buf, off = ta.pack_documents(v["docs"])
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(v["docs"]), int(off[-1]), stream=torch.cuda.current_stream().cuda_stream).sync()
    ids = b.ids_tensor().cpu().numpy().view("uint32")
    tof = b.tok_offsets_tensor().cpu().numpy()
    for i in range(len(v["docs"])):
        assert ids[tof[i]:tof[i + 1]].tolist() == v["ids"][i]


def test_same_device_twice():
    v = load_vectors("spm_bpe_llama2")
    tok = _tok("spm_bpe_llama2")
    two = ta.Tokenizer.from_str(load_tokenizer_json("spm_bpe_llama2"), device=[0, 0])
    docs = v["docs"] * 3
    a = tok.encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)


@pytest.mark.parametrize("name", NAMES)
def test_decode_round_trip(name):
    v = load_vectors(name)
    tok = _tok(name)
    assert tok.decode_batch(v["ids"], skip_special_tokens=False) == v["decoded"]
    got = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert tok.decode_batch([list(got[i].ids) for i in range(len(v["docs"]))], skip_special_tokens=False) == v["decoded"]


@pytest.mark.parametrize("name", NAMES)
def test_units_beyond_8kb(name):
    """Units longer than the LDS kernels' 8 KB (a 10,000-char CJK run, a 20 KB blob without spaces, documents and units of exactly
    8,192 / 8,193 bytes) run in k_bpe_merge_huge: bit-exact, no error flag."""
    v = load_vectors("spm_bpe_long")
    exp = v[name]
    docs = v["docs"]
    tok = _tok(name)
    got = tok.encode_batch(docs, add_special_tokens=False)
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    fast = tok.encode_batch_fast(docs, add_special_tokens=False)
    for k, d in enumerate(docs):
        words = exp["words"][k] if "words" in exp else [0] * len(exp["ids"][k])
        offs = [tuple(exp["offsets_char"][k][2 * j:2 * j + 2]) for j in range(len(exp["ids"][k]))]
        assert list(got[k].ids) == exp["ids"][k], (name, k)
        assert [tuple(o) for o in got[k].offsets] == offs, (name, k)
        assert list(got[k].word_ids) == words, (name, k)
        m = char_to_byte(d)
        a, z = _csr(b, k)
        assert b.ids[a:z].tolist() == exp["ids"][k], (name, k)
        assert b.offsets[a:z].tolist() == [[m[x], m[y]] for x, y in offs], (name, k)
        assert b.word_ids[a:z].tolist() == words, (name, k)
        assert list(fast[k].ids) == exp["ids"][k], (name, k)


def test_char_bpe_words_beyond_8kb(ref_tokenizers):
    """The same kernel serves BPE over characters behind Whitespace: a word of more than 8 KB is encoded, no longer refused."""
    from tests.helpers import load_tokenizer_json as lj
    js = lj("bpe_ws_byte_fallback")
    tok = ta.Tokenizer.from_str(js, device=0)
    w = ref_tokenizers.Tokenizer.from_str(js)
    rng = random.Random(7)
    docs = ["x" * 9000, "中" * 4000 + " tail", "".join(rng.choice("abcdefgh中é😀") for _ in range(12000)), "short words here"]
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    for k in range(len(docs)):
        assert list(got[k].ids) == exp[k].ids, k
        assert [tuple(o) for o in got[k].offsets] == exp[k].offsets, k


def test_normalized_added_tokens_behind_metaspace(ref_tokenizers):
    """normalized = true added tokens with Metaspace (no normalizer): matched by the second pass over the raw pieces."""
    import json
    d = json.loads(load_tokenizer_json("spm_bpe_first"))
    nxt = max(d["model"]["vocab"].values()) + 1
    for k, c in enumerate(["<x>", "hello", " ok"]):
        d["added_tokens"].append({"id": nxt + k, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False})
    js = json.dumps(d, ensure_ascii=False)
    tok = ta.Tokenizer.from_str(js, device=0)
    w = ref_tokenizers.Tokenizer.from_str(js)
    docs = ["a<x>b hello c", "hello", " ok ok", "<s>hello<x></s> x", "no tokens here", "hellohello <x><x>"]
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    for k, doc in enumerate(docs):
        assert list(got[k].ids) == exp[k].ids, doc
        assert [tuple(o) for o in got[k].offsets] == exp[k].offsets, doc
        assert list(got[k].word_ids) == exp[k].word_ids, doc


def _random_docs(rng, n):
    pool = ["a", "b", "the", "ing", " ", "  ", "\t", "\n", MS, "<s>", "</s>", "<unk>", "中", "文字", "😀", "ꙮ", "é", "ß", "Hello", "world", ",", ".",
            "x", "12", "ё", "ﬁ", "​"]
    return ["".join(rng.choice(pool) for _ in range(rng.randint(0, 30))) for _ in range(n)]


@pytest.mark.parametrize("name", NAMES)
def test_live_differential(name, ref_tokenizers):
    w = ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name))
    tok = _tok(name)
    from oracle import synth
    rng = random.Random(101 + NAMES.index(name))
    docs = _random_docs(rng, N(3000)) + synth.gen_lines(N(1000), text_seed=77)
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
