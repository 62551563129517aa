"""BLOOM's Split + ByteLevel(use_regex=false) on the device (kernels/pretok_bloom.hip) against the reference wheel's vectors
(tools/make_golden_bloom.py): every array through every entry, and documents built so that one of the 39 chars the pattern's class leaves
out, a space in front of a class char or a wide char sits where the lane kernel can go wrong (tests/bloom_cases.py).  Behind the start
mask nothing knows which rule made it: segments cut by added tokens, words, pairs, mixed batches, truncation, padding, overflow and
decode are held to the wheel's answers all the same.  Also the Gemma-2 / Gemma-3 layout -- Split(String " ", MergedWithPrevious) behind
the U+2581 normalizers, which loads as the "▁" front -- against the vectors of the same files with a null pre-tokenizer.  Under
TKAMD_SIMT=1 all of this is the CPU rehearsal."""
import json

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import bloom_cases as bc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

GEMMA_SPLIT = {"type": "Split", "pattern": {"String": " "}, "behavior": "MergedWithPrevious", "invert": False}


@pytest.fixture(scope="module")
def v():
    return load_vectors(bc.NAME)


@pytest.fixture(scope="module")
def tok():
    return _tok()


def _tok(**kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(bc.NAME), device=0, **kw)


def _pairs(flat):
    return [(flat[2 * j], flat[2 * j + 1]) for j in range(len(flat) // 2)]


def _csr(b, i):
    return int(b.tok_offsets[i]), int(b.tok_offsets[i + 1])


def _hold(got, exp, docs, fields=("ids", "offsets_char", "words")):
    for i, d in enumerate(docs):
        e = got[i]
        assert list(e.ids) == exp["ids"][i], (i, d[-24:])
        if "offsets_char" in fields:
            assert [tuple(o) for o in e.offsets] == _pairs(exp["offsets_char"][i]), (i, d[-24:])
        if "words" in fields:
            assert list(e.word_ids) == exp["words"][i], (i, d[-24:])
        if "type_ids" in fields:
            assert list(e.type_ids) == exp["type_ids"][i], (i, d[-24:])


def _hold_csr(b, exp, docs):
    """the CSR itself, ids, byte offsets and word ids of a CSR batch"""
    assert np.diff(b.tok_offsets[:len(docs) + 1]).tolist() == [len(x) for x in exp["ids"][:len(docs)]]
    for i, d in enumerate(docs):
        a, z = _csr(b, i)
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == exp["ids"][i], (i, d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(exp["offsets_char"][i])], (i, d[-24:])
        assert b.word_ids[a:z].tolist() == exp["words"][i], (i, d[-24:])


def _pick(exp, idx):
    return {k: [exp[k][i] for i in idx] for k in ("ids", "offsets_char", "words")}


def test_singles_every_array(tok, v):
    docs = v["docs"]
    short = bc.short_docs()
    assert docs[:len(short)] == short                     # (the shapes of tests/bloom_cases.py are what the vectors hold)
    assert any(bc.USER in d for d in docs) and any(bc.EOS in d for d in docs)      # segments cut by added tokens, special and not
    _hold(tok.encode_batch(docs, add_special_tokens=False), v, docs)
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), v, docs)


def test_short_documents_alone_at_byte_0(tok, v):
    """every short document alone, so that a space that is its last byte, or one of the 39 that is its only char, ends the text"""
    short = bc.short_docs()
    for i, d in enumerate(short[:120]):
        _hold(tok.encode_batch([d], add_special_tokens=False), _pick(v, [i]), [d])


def test_empty_documents_and_spaces_at_document_ends(tok, v):
    for docs, exp in zip(bc.batches(), v["batches"]):
        _hold(tok.encode_batch(docs, add_special_tokens=False), exp, docs)
        _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), exp, docs)


def test_fast_and_packed_entries(tok, v):
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert [list(e.ids) for e in fast] == v["ids"]
    buf, off = ta.pack_documents(v["docs"])
    b = tok.encode_packed(buf, off)
    for i in range(len(v["docs"])):
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i], i


@pytest.mark.needs_hw
def test_device_entry(tok, v):
    import torch
    buf, off = ta.pack_documents(v["docs"])
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(v["docs"]), int(off[-1]), stream=torch.cuda.current_stream().cuda_stream).sync()
    ids = b.ids_tensor().cpu().numpy().view("uint32")
    assert ids.tolist() == [x for e in v["ids"] for x in e]


@pytest.mark.parametrize("k", range(len(bc.FAMILIES)))
def test_edge_document_alone_and_with_its_neighbours(k, tok, v):
    """one document of 16384 + 72 bytes per edge family: alone at byte 0 of the text, so that its pattern sits at exactly the bytes of
    the mask word, the wavefront and the workgroup it was built for -- char offsets (the lead-byte mask rides in the lane kernel) and
    byte offsets -- and as a batch of three with its neighbours, which moves it by 8 bytes a document"""
    docs = bc.device_edge_docs()
    assert len(docs) == len(v["edge"]["ids"]) and all(len(d.encode("utf-8")) == 16384 + 72 for d in docs)
    exp = _pick(v["edge"], [k])
    _hold(tok.encode_batch([docs[k]], add_special_tokens=False), exp, [docs[k]])
    _hold_csr(tok.encode_batch_csr([docs[k]], offsets="byte", word_ids=True), exp, [docs[k]])
    idx = [(k - 1) % len(docs), k, (k + 1) % len(docs)]
    three = [docs[i] for i in idx]
    _hold(tok.encode_batch(three, add_special_tokens=False), _pick(v["edge"], idx), three)
    _hold_csr(tok.encode_batch_csr(three, offsets="byte", word_ids=True), _pick(v["edge"], idx), three)


def test_one_document_of_70_kb_and_a_small_batch_behind_a_large_one(tok, v):
    """several workgroups of the lane kernel; then a small batch on the same handle, whose buffers the large one left behind"""
    big = bc.big_doc()
    assert len(big.encode("utf-8")) == v["big"]["n_bytes"] > 65536
    e = tok.encode_batch([big, "x "], add_special_tokens=False)
    _hold(e, v["big"], [big])
    assert list(e[1].ids) == v["ids"][v["docs"].index("x ")]
    b = tok.encode_batch_csr([big], offsets="none")              # (ids only, the document alone)
    assert b.ids.tolist() == v["big"]["ids"][0]
    small = v["docs"][:9]
    _hold(tok.encode_batch(small, add_special_tokens=False), v, small)
    _hold_csr(tok.encode_batch_csr(small, offsets="byte", word_ids=True), v, small)


def test_pairs_and_a_mixed_batch(tok, v):
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    _hold(got, v["pairs"], [p[0] for p in pairs], fields=("ids", "offsets_char", "words", "type_ids"))
    for i in range(len(pairs)):
        assert list(got[i].sequence_ids) == v["pairs"]["sequence_ids"][i]
    items, exp = [], []
    for i in range(min(40, len(pairs))):
        k = v["docs"].index(pairs[i][0])
        items.append(pairs[i][0]); exp.append(v["ids"][k])              # (no template: with special tokens the ids are the same)
        items.append(pairs[i]); exp.append(v["pairs"]["ids"][i])
    got = tok.encode_batch(items, add_special_tokens=True)
    for i in range(len(items)):
        assert list(got[i].ids) == exp[i], items[i]


def test_pretokenized_input(tok, v):
    p = v["pretok"]
    _hold(tok.encode_batch(p["inputs"], is_pretokenized=True, add_special_tokens=False), p, [" ".join(w) for w in p["inputs"]])


def test_encode_special_tokens(v):
    t = _tok()
    t.encode_special_tokens = True
    _hold(t.encode_batch(v["docs"], add_special_tokens=False), v["encode_special"], v["docs"])
    k = v["docs"].index("a " + bc.USER + "b")             # (not special: matched all the same)
    assert v["encode_special"]["ids"][k] == v["ids"][k]
    k = v["docs"].index("a " + bc.EOS)                    # (special: read as text)
    assert len(v["encode_special"]["ids"][k]) > len(v["ids"][k])


def test_truncation_with_a_stride_and_overflowing(v):
    t = _tok()
    t.enable_truncation(max_length=v["trunc"]["max_length"], stride=v["trunc"]["stride"])
    got = t.encode_batch_csr(v["docs"], add_special_tokens=True, offsets="char", overflowing=True)
    for i, d in enumerate(v["docs"]):
        e = got[i]
        assert list(e.ids) == v["trunc"]["ids"][i], (i, d[-24:])
        assert [tuple(o) for o in e.offsets] == _pairs(v["trunc"]["offsets_char"][i]), (i, d[-24:])
        assert [list(o.ids) for o in e.overflowing] == v["trunc"]["overflowing"][i], (i, d[-24:])
        assert [[tuple(x) for x in o.offsets] for o in e.overflowing] == [_pairs(f) for f in v["trunc"]["overflowing_offsets_char"][i]], (i, d[-24:])
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = t.encode_batch_csr(pairs, add_special_tokens=True, overflowing=True)
    for i in range(len(pairs)):
        assert list(got[i].ids) == v["trunc"]["pair_ids"][i], pairs[i]
        assert [list(o.ids) for o in got[i].overflowing] == v["trunc"]["pair_overflowing"][i], pairs[i]


def test_padding_of_both_kinds(v):
    small = [d for d in v["docs"] if len(d) < 120]
    t = _tok()
    t.enable_padding(pad_id=v["pad"]["pad_id"], pad_token=bc.PAD)
    got = t.encode_batch(small, add_special_tokens=True)
    for i, d in enumerate(small):
        assert list(got[i].ids) == v["pad"]["ids"][i] and list(got[i].attention_mask) == v["pad"]["attention_mask"][i], (i, d[-24:])
        assert [tuple(o) for o in got[i].offsets] == _pairs(v["pad"]["offsets_char"][i]), (i, d[-24:])
    t = _tok()
    t.enable_truncation(max_length=v["pad_fixed_left"]["length"])
    t.enable_padding(pad_id=v["pad"]["pad_id"], pad_token=bc.PAD, length=v["pad_fixed_left"]["length"], direction="left")
    got = t.encode_batch(small, add_special_tokens=True)
    for i, d in enumerate(small):
        assert list(got[i].ids) == v["pad_fixed_left"]["ids"][i] and list(got[i].attention_mask) == v["pad_fixed_left"]["attention_mask"][i], (i, d[-24:])
        assert list(got[i].special_tokens_mask) == v["pad_fixed_left"]["special_tokens_mask"][i], (i, d[-24:])


def test_decode_round_trip(tok, v):
    assert tok.decode_batch(v["ids"], skip_special_tokens=False) == v["decoded"]
    assert tok.decode_batch(v["ids"], skip_special_tokens=True) == v["decoded_skip"]
    got = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert tok.decode_batch([list(e.ids) for e in got], skip_special_tokens=False) == v["decoded"]
    plain = [d for d in v["docs"] if "<" not in d]
    assert len(plain) > 300
    assert [v["decoded"][v["docs"].index(d)] for d in plain] == plain          # (byte-level: the text comes back as it went in)


def test_empty_batch_and_empty_documents(tok):
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0
    got = tok.encode_batch(["", ""], add_special_tokens=False)
    assert len(got[0].ids) == 0 and len(got[1].ids) == 0
    b = tok.encode_batch_csr(["", "x ", "", ""], offsets="byte", word_ids=True)
    assert b.tok_offsets.tolist()[:2] == [0, 0] and b.tok_offsets[2] == b.tok_offsets[4] == 2
    assert b.word_ids.tolist() == [0, 1]
    assert b.offsets.tolist() == [[0, 1], [1, 2]]


def test_same_device_twice(v):
    two = ta.Tokenizer.from_str(load_tokenizer_json(bc.NAME), device=[0, 0])
    docs = v["docs"] * 2
    a = _tok().encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)


@pytest.mark.parametrize("name", ["spm_bpe_llama2", "spm_bpe_replace_only"])
def test_gemma_split_files_against_the_vectors_of_the_null_pre_tokenizer(name):
    """Split(String " ", MergedWithPrevious) behind the U+2581 normalizers is inert: the vectors the wheel wrote for the same file with
    pre_tokenizer null hold for it, array by array"""
    d = json.loads(load_tokenizer_json(name))
    assert d["pre_tokenizer"] is None
    d["pre_tokenizer"] = GEMMA_SPLIT
    tok = ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=0)
    assert tok.info["pre_tokenizer"] == 7 and tok.info["normalizer"] == 2
    v = load_vectors(name)
    got = tok.encode_batch(v["docs"], add_special_tokens=False)
    b = tok.encode_batch_csr(v["docs"], offsets="byte", word_ids=True)
    for i, doc in enumerate(v["docs"]):
        e = got[i]
        assert list(e.ids) == v["ids"][i], (name, doc)
        assert [list(o) for o in e.offsets] == v["offsets_char"][i], (name, doc)
        assert list(e.word_ids) == v["words"][i], (name, doc)
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i], (name, doc)
        assert b.offsets[a:z].tolist() == v["offsets"][i], (name, doc)
        assert b.word_ids[a:z].tolist() == v["words"][i], (name, doc)
