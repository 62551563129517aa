"""Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family on the device (kernels/pretok_digits.hip) against the reference
wheel's vectors (tools/make_golden_digits.py): every array through every entry, and documents built so that a numeric char, a whitespace
run or a contraction sits where the lane kernel can go wrong (tests/digits_cases.py).  Behind the start mask nothing knows which rule made
it: segments cut by added tokens, words, pairs, mixed batches, truncation, padding, overflow and decode are held to the wheel's answers
all the same.  digits_individual gets the full set, digits_contiguous the singles and the edge documents.  Also the CPU rehearsal of all
this under TKAMD_SIMT=1."""
import json

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import digits_cases as dc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

IND, CON = dc.NAMES


@pytest.fixture(scope="module")
def vectors():
    return {name: load_vectors(name) for name in dc.NAMES}


@pytest.fixture(scope="module")
def toks():
    return {name: _tok(name) for name in dc.NAMES}


@pytest.fixture(scope="module")
def v(vectors):
    return vectors[IND]


@pytest.fixture(scope="module")
def tok(toks):
    return toks[IND]


def _tok(name=IND, **kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(name), device=0, **kw)


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
        if "special_tokens_mask" in fields:
            assert list(e.special_tokens_mask) == exp["special_tokens_mask"][i], (i, d[-24:])


def _hold_csr(b, exp, docs):
    """ids, byte offsets and word ids of a CSR batch"""
    for i, d in enumerate(docs):
        a, z = _csr(b, i)
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == exp["ids"][i], (i, d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(exp["offsets_char"][i])], (i, d[-24:])
        assert b.word_ids[a:z].tolist() == exp["words"][i], (i, d[-24:])


@pytest.mark.parametrize("name", dc.NAMES)
def test_singles_every_array(name, toks, vectors):
    tok, v = toks[name], vectors[name]
    docs = v["docs"]
    short = [d for d in dc.edge_docs() if len(d) < 400]
    assert docs[:len(short)] == short                     # (the shapes of tests/digits_cases.py are what the vectors hold)
    _hold(tok.encode_batch(docs, add_special_tokens=False), v, docs)
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), v, docs)


@pytest.mark.parametrize("name", dc.NAMES)
def test_each_edge_document_alone_at_byte_0(name, toks, vectors):
    """alone at byte 0 of the text, so that its numeric char sits at exactly the byte of the mask word, the wavefront and the workgroup
    it was built for: char offsets (the lead-byte mask rides in the lane kernel) for every one, byte offsets for the long ones"""
    tok, v = toks[name], vectors[name]
    docs = dc.edge_docs()
    assert len(docs) == len(v["edge"]["ids"])
    for i, d in enumerate(docs):
        exp = {k: [v["edge"][k][i]] for k in ("ids", "offsets_char", "words")}
        _hold(tok.encode_batch([d], add_special_tokens=False), exp, [d])
        if len(d) >= 400:
            _hold_csr(tok.encode_batch_csr([d], offsets="byte", word_ids=True), exp, [d])


@pytest.mark.parametrize("name", dc.NAMES)
def test_empty_documents_between_digit_documents(name, toks, vectors):
    tok, v = toks[name], vectors[name]
    for docs, exp in zip(dc.batches(), v["batches"]):
        _hold(tok.encode_batch(docs, add_special_tokens=False), exp, docs)
        _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), exp, docs)


@pytest.mark.parametrize("name", dc.NAMES)
def test_fast_and_packed_entries(name, toks, vectors):
    tok, v = toks[name], vectors[name]
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert [list(e.ids) for e in fast] == v["ids"]
    buf, off = ta.pack_documents(v["docs"])
    b = tok.encode_packed(buf, off)
    for i in range(len(v["docs"])):
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i], i


@pytest.mark.parametrize("name", dc.NAMES)
def test_one_document_of_70_kb(name, toks, vectors):
    """several workgroups of the lane kernel"""
    tok, v = toks[name], vectors[name]
    big = dc.big_doc()
    assert len(big.encode("utf-8")) == v["big"]["n_bytes"] > 65536
    e = tok.encode_batch([big, "a  1"], add_special_tokens=False)
    _hold(e, v["big"], [big])
    assert len(e[1].ids) == 3
    b = tok.encode_batch_csr([big], offsets="none")              # (ids only, the document alone)
    assert b.ids.tolist() == v["big"]["ids"][0]


def test_with_special_tokens(tok, v):
    _hold(tok.encode_batch(v["docs"], add_special_tokens=True), v["special"], v["docs"], fields=("ids", "offsets_char", "words", "type_ids", "special_tokens_mask"))


def test_pairs_and_a_mixed_batch(tok, v):
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    _hold(got, v["pairs"], [p[0] for p in pairs], fields=("ids", "offsets_char", "words", "type_ids", "special_tokens_mask"))
    for i in range(len(pairs)):
        assert list(got[i].sequence_ids) == v["pairs"]["sequence_ids"][i]
    small = [d for d in v["docs"] if len(d) < 120]
    assert [p[0] for p in pairs] == small[::2]
    items, exp = [], []
    for i in range(min(40, len(pairs))):
        k = v["docs"].index(small[i])
        items.append(small[i]); exp.append(v["special"]["ids"][k])
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
    k = v["docs"].index(dc.USER + "7")                  # (not special: matched all the same)
    assert v["encode_special"]["ids"][k] == v["ids"][k] and len(v["ids"][k]) == 2
    k = v["docs"].index("12" + dc.EOS + "34")           # (special: read as text)
    assert len(v["encode_special"]["ids"][k]) > len(v["ids"][k]) == 5


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
    t.enable_padding(pad_id=v["pad"]["pad_id"], pad_token=dc.PAD)
    got = t.encode_batch(small, add_special_tokens=True)
    for i, d in enumerate(small):
        assert list(got[i].ids) == v["pad"]["ids"][i] and list(got[i].attention_mask) == v["pad"]["attention_mask"][i], (i, d[-24:])
        assert [tuple(o) for o in got[i].offsets] == _pairs(v["pad"]["offsets_char"][i]), (i, d[-24:])
    t = _tok()
    t.enable_truncation(max_length=v["pad_fixed_left"]["length"])
    t.enable_padding(pad_id=v["pad"]["pad_id"], pad_token=dc.PAD, length=v["pad_fixed_left"]["length"], direction="left")
    got = t.encode_batch(small, add_special_tokens=True)
    for i, d in enumerate(small):
        assert list(got[i].ids) == v["pad_fixed_left"]["ids"][i] and list(got[i].attention_mask) == v["pad_fixed_left"]["attention_mask"][i], (i, d[-24:])
        assert list(got[i].special_tokens_mask) == v["pad_fixed_left"]["special_tokens_mask"][i], (i, d[-24:])


def test_decode_round_trip(tok, v):
    assert tok.decode_batch(v["ids"], skip_special_tokens=False) == v["decoded"]
    assert tok.decode_batch(v["ids"], skip_special_tokens=True) == v["decoded_skip"]
    got = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert tok.decode_batch([list(e.ids) for e in got], skip_special_tokens=False) == v["decoded"]
    plain = [d for d in v["docs"] if "<|" not in d]
    assert len(plain) > 300
    assert [v["decoded"][v["docs"].index(d)] for d in plain] == plain          # (byte-level: the text comes back as it went in)


def test_empty_batch_and_empty_documents(tok):
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0
    got = tok.encode_batch(["", ""], add_special_tokens=False)
    assert len(got[0].ids) == 0 and len(got[1].ids) == 0
    b = tok.encode_batch_csr(["", "a  1", "", ""], offsets="byte", word_ids=True)
    assert b.tok_offsets.tolist()[:2] == [0, 0] and b.tok_offsets[2] == b.tok_offsets[4] == 3
    assert b.word_ids.tolist() == [0, 1, 2]
    assert b.offsets.tolist() == [[0, 1], [1, 3], [3, 4]]


def test_nfc_in_front_goes_through_the_general_path(v):
    """normalizer NFC in front: on text that is NFC already the result is the vectors' (with and without speculation); one decomposed
    document sends the batch through the normalizer's kernels, and Digits then reads the normalized text"""
    d = json.loads(load_tokenizer_json(IND))
    d["normalizer"] = {"type": "NFC"}
    t = ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=0)
    import unicodedata
    idx = [i for i, x in enumerate(v["docs"]) if unicodedata.is_normalized("NFC", x) and all(ord(c) < 0x300 or ord(c) > 0x36F for c in x) and len(x) < 200]
    assert len(idx) > 100
    docs = [v["docs"][i] for i in idx]
    for _ in range(2):
        got = t.encode_batch(docs, add_special_tokens=False)
        for k, i in enumerate(idx):
            assert list(got[k].ids) == v["ids"][i], docs[k][-24:]
            assert [tuple(o) for o in got[k].offsets] == _pairs(v["offsets_char"][i]), docs[k][-24:]
    nfc = v["nfc"]
    assert not all(unicodedata.is_normalized("NFC", x) for x in nfc["docs"])
    _hold(t.encode_batch(nfc["docs"], add_special_tokens=False), nfc, nfc["docs"])


def test_same_device_twice(v):
    two = ta.Tokenizer.from_str(load_tokenizer_json(IND), device=[0, 0])
    docs = v["docs"] * 2
    a = _tok().encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)
