"""The chained Split pre-tokenizer of DeepSeek-V3 / R1 on the device (kernels/pretok_ds3.hip) against the reference wheel's vectors
(tools/make_golden_split_chain.py): every array through every entry, and documents built so that a run, a piece edge or a wide char sits
where the lane kernel and the sequential matcher behind it can go wrong (tests/split_chain_cases.py).  Behind the start mask nothing
knows which rule made it: segments cut by added tokens, words, pairs, mixed batches, truncation, padding, overflow and decode are held to
the wheel's answers all the same.  Also the CPU rehearsal of all this under TKAMD_SIMT=1."""
import json

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import split_chain_cases as sc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAME = "ds3_chain"


@pytest.fixture(scope="module")
def v():
    return load_vectors(NAME)


@pytest.fixture(scope="module")
def tok():
    return _tok()


def _tok(**kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(NAME), device=0, **kw)


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


def test_singles_every_array(tok, v):
    docs = v["docs"]
    assert docs == sc.edge_docs() + docs[len(sc.edge_docs()):]          # (the shapes of tests/split_chain_cases.py are what the vectors hold)
    _hold(tok.encode_batch(docs, add_special_tokens=False), v, docs)
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    for i, d in enumerate(docs):
        a, z = _csr(b, i)
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == v["ids"][i], (i, d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(v["offsets_char"][i])], (i, d[-24:])
        assert b.word_ids[a:z].tolist() == v["words"][i], (i, d[-24:])


def test_each_edge_document_first_in_its_batch(tok, v):
    """alone at byte 0 of the text, so that its run sits at exactly the window byte it was built for; with a neighbour behind it"""
    n = len(sc.edge_docs())
    for i in range(n):
        d = v["docs"][i]
        b = tok.encode_batch_csr([d, "tail 12"], offsets="byte", word_ids=True)
        a, z = _csr(b, 0)
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == v["ids"][i], (i, d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(v["offsets_char"][i])], (i, d[-24:])
        assert b.word_ids[a:z].tolist() == v["words"][i], (i, d[-24:])


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
    k = v["docs"].index(sc.USER)                        # (not special: matched all the same)
    assert v["encode_special"]["ids"][k] == v["ids"][k] and len(v["ids"][k]) == 1
    k = v["docs"].index("tail  " + sc.EOS + "  head")   # (special: read as text)
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
    t.enable_padding(pad_id=v["pad"]["pad_id"], pad_token=sc.PAD)
    got = t.encode_batch(small, add_special_tokens=True)
    for i, d in enumerate(small):
        assert list(got[i].ids) == v["pad"]["ids"][i] and list(got[i].attention_mask) == v["pad"]["attention_mask"][i], (i, d[-24:])
        assert [tuple(o) for o in got[i].offsets] == _pairs(v["pad"]["offsets_char"][i]), (i, d[-24:])
    t = _tok()
    t.enable_truncation(max_length=v["pad_fixed_left"]["length"])
    t.enable_padding(pad_id=v["pad"]["pad_id"], pad_token=sc.PAD, length=v["pad_fixed_left"]["length"], direction="left")
    got = t.encode_batch(small, add_special_tokens=True)
    for i, d in enumerate(small):
        assert list(got[i].ids) == v["pad_fixed_left"]["ids"][i] and list(got[i].attention_mask) == v["pad_fixed_left"]["attention_mask"][i], (i, d[-24:])
        assert list(got[i].special_tokens_mask) == v["pad_fixed_left"]["special_tokens_mask"][i], (i, d[-24:])


def test_fast_and_packed_entries(tok, v):
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert [list(e.ids) for e in fast] == v["ids"]
    buf, off = ta.pack_documents(v["docs"])
    b = tok.encode_packed(buf, off)
    for i in range(len(v["docs"])):
        a, z = _csr(b, i)
        assert b.ids[a:z].tolist() == v["ids"][i], i


def test_decode_round_trip(tok, v):
    assert tok.decode_batch(v["ids"], skip_special_tokens=False) == v["decoded"]
    assert tok.decode_batch(v["ids"], skip_special_tokens=True) == v["decoded_skip"]
    got = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert tok.decode_batch([list(e.ids) for e in got], skip_special_tokens=False) == v["decoded"]
    plain = [d for d in v["docs"] if "<｜" not in d]
    assert [v["decoded"][v["docs"].index(d)] for d in plain] == plain          # (byte-level: the text comes back as it went in)


def test_empty_batch_and_empty_documents(tok):
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0
    got = tok.encode_batch(["", ""], add_special_tokens=False)
    assert len(got[0].ids) == 0 and len(got[1].ids) == 0
    b = tok.encode_batch_csr(["", "a  1", "", ""], offsets="byte", word_ids=True)
    assert b.tok_offsets.tolist()[:2] == [0, 0] and b.tok_offsets[2] == b.tok_offsets[4] == 3
    assert b.word_ids.tolist() == [0, 1, 2]


def test_one_document_of_70_kb(tok, v):
    """several workgroups of the lane kernel; the document holds undecided bytes, so the sequential matcher redoes all of it"""
    big = sc.big_doc()
    assert len(big.encode("utf-8")) == v["big"]["n_bytes"] > 65536
    e = tok.encode_batch([big, "a  1"], add_special_tokens=False)
    assert list(e[0].ids) == v["big"]["ids"]
    assert [tuple(o) for o in e[0].offsets] == _pairs(v["big"]["offsets_char"])
    assert list(e[0].word_ids) == v["big"]["words"]
    assert len(e[1].ids) == 3
    b = tok.encode_batch_csr([big], offsets="none")              # (ids only, the document alone)
    assert b.ids.tolist() == v["big"]["ids"]


def test_short_batches_with_a_short_and_with_an_empty_list_for_the_sequential_matcher(tok, v):
    for key, docs in (("short_batch", sc.short_batch()), ("plain_batch", sc.plain_batch())):
        got = tok.encode_batch_fast(docs, add_special_tokens=False)
        assert [list(e.ids) for e in got] == v[key]["ids"], key
        n_slow = tok.queue_sizes()["pretok_slow_docs"]                   # documents the lane kernel handed to the sequential matcher
        assert (5 <= n_slow <= 30) if key == "short_batch" else n_slow == 0, (key, n_slow)
        got = tok.encode_batch(docs, add_special_tokens=False)           # (char offsets: the lead-byte mask rides in the lane kernel)
        assert [list(e.ids) for e in got] == v[key]["ids"], key


def test_nfc_in_front_goes_through_the_general_path(v):
    """normalizer NFC in front of the chain: on text that is NFC already the result is the vectors' (with and without speculation)"""
    d = json.loads(load_tokenizer_json(NAME))
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
    # one document that is not NFC sends the batch through the normalizer's kernels: the chain then reads the normalized text
    got = t.encode_batch(docs[:20] + ["é  12"], add_special_tokens=False)
    for k in range(20):
        assert list(got[k].ids) == v["ids"][idx[k]]
    plain = _tok().encode_batch(["é  12"], add_special_tokens=False)[0]
    assert list(got[20].ids) == list(plain.ids)


def test_same_device_twice(v):
    two = ta.Tokenizer.from_str(load_tokenizer_json(NAME), device=[0, 0])
    docs = v["docs"] * 2
    a = _tok().encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)
