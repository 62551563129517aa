"""The CLIP layout on the device: Sequence[NFC, Replace(\\s+), Lowercase] (the NFC_LOWER mode of csrc/nfc_core.hpp), Split(the CLIP pattern,
Removed, inverted) + ByteLevel (k_pretok_clip: a start AND an end mask) and byte-level BPE with end_of_word_suffix "</w>" (the last byte
of a word seeded from DevTables::byte_sfx in every merge tier) -- every array against the wheel's vectors (tools/make_golden_clip.py) of
documents built so that a contraction, an O run ending in ', a digit, a 4-byte char and a char that lowercases to two sit where the
kernels can go wrong: ending at and straddling a lane's 64-byte word, a wavefront's 4,096 bytes and the workgroup's 16,384; first and
last in a document; as the last bytes of the batch.  tests/test_clip.py runs these very functions under the SIMT emulation."""
import json

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import clip_cases as cc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAME, PLAIN = cc.NAMES
_VECTORS = {}


def _v(name=NAME):
    if name not in _VECTORS:
        v = load_vectors(name)
        v["at"] = {d: i for i, d in reversed(list(enumerate(v["docs"])))}
        _VECTORS[name] = v
    return _VECTORS[name]


def _tok(name=NAME, **kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(name), device=0, **kw)


def _pairs(flat):
    return [(flat[2 * j], flat[2 * j + 1]) for j in range(len(flat) // 2)]


def _hold_csr(b, docs, v, what=""):
    """ids, byte offsets, word ids of a CSR result against the vectors"""
    for k, d in enumerate(docs):
        i = v["at"][d]
        a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == v["ids"][i], (what, k, len(d), d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(v["offsets_char"][i])], (what, k, len(d), d[-24:])
        assert b.word_ids[a:z].tolist() == v["words"][i], (what, k, len(d), d[-24:])


def _hold_encodings(got, docs, v, what=""):
    for k, d in enumerate(docs):
        i = v["at"][d]
        assert list(got[k].ids) == v["ids"][i], (what, k, len(d), d[-24:])
        assert [tuple(o) for o in got[k].offsets] == _pairs(v["offsets_char"][i]), (what, k, len(d), d[-24:])
        assert list(got[k].word_ids) == v["words"][i], (what, k, len(d), d[-24:])


def test_vectors_every_array():
    """the whole batch at once: more than two workgroups of text, a document count that is no multiple of 256"""
    v = _v()
    tok = _tok()
    docs = v["docs"]
    assert tok.info["pre_tokenizer"] == 10 and tok.info["normalizer"] == 7 and tok.info["model"] == 1
    assert docs == cc.all_docs() and len(docs) % 256 and sum(len(d.encode("utf-8")) for d in docs) > 2 * 16384
    _hold_encodings(tok.encode_batch(docs, add_special_tokens=False), docs, v)
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v)
    fast = tok.encode_batch_fast(docs, add_special_tokens=False)
    assert [list(e.ids) for e in fast] == v["ids"]
    # a second time on the same handle (the normalizer's speculation has settled by now), and last to first
    back = docs[::-1]
    _hold_csr(tok.encode_batch_csr(back, offsets="byte", word_ids=True), back, v, what="reversed")


def test_edge_documents_each_first_in_a_batch_of_its_own():
    """the atom sits at exactly that byte of the text; with a tail document behind it, and as the last bytes of the batch"""
    v = _v()
    tok = _tok()
    edge = cc.edge_docs()
    assert len(edge) > 300
    for d in edge:
        _hold_csr(tok.encode_batch_csr([d], offsets="byte", word_ids=True), [d], v, what="alone")
    for d in edge[::7]:
        docs = [d, "tail it's", ""]
        _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs[:1], v, what="with a tail")
        _hold_encodings(tok.encode_batch([d], add_special_tokens=False), [d], v, what="char offsets")


def test_runs_whitespace_only_and_empty_documents():
    """300 digits (300 pre-tokens), 300 apostrophes (one), a 9 KB letter run (the huge merge tier, its last byte suffixed), whitespace alone"""
    v = _v()
    tok = _tok()
    docs = cc.run_docs()
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    _hold_csr(b, docs, v)
    n = [int(b.tok_offsets[k + 1] - b.tok_offsets[k]) for k in range(len(docs))]
    words = [b.word_ids[int(b.tok_offsets[k]):int(b.tok_offsets[k + 1])].tolist() for k in range(len(docs))]
    assert words[0] == list(range(300)) and set(words[2]) == {0} and set(words[6]) == {0} and len(docs[6].encode("utf-8")) > 8192
    assert [n[docs.index(d)] for d in (" ", "   ", "\n\t \u00a0\u3000", "")] == [0, 0, 0, 0]      # (U+001C and U+200B are no \s chars: tokens, as the vectors have them)
    for d in docs:                                         # ... and each first in a batch of its own
        _hold_csr(tok.encode_batch_csr([d, "x"], offsets="byte", word_ids=True), [d], v, what="alone")
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0
    assert [len(e.ids) for e in tok.encode_batch(["", " ", ""], add_special_tokens=False)] == [0, 0, 0]


def test_the_last_byte_of_a_word_decides_the_id():
    v = _v()
    tok = _tok()
    vocab = json.loads(load_tokenizer_json(NAME))["model"]["vocab"]
    docs = cc.last_byte_docs()
    got = tok.encode_batch(docs, add_special_tokens=False)
    _hold_encodings(got, docs, v)
    assert list(got[docs.index("a")].ids) == [vocab["a</w>"]] and vocab["a"] not in list(got[docs.index("a a")].ids)
    assert list(got[docs.index("the")].ids) == [vocab["the</w>"]] and list(got[docs.index("the the")].ids) == [vocab["the</w>"]] * 2
    assert list(got[docs.index("'red")].ids) == [vocab["'re</w>"], vocab["d</w>"]]
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v)


def test_added_tokens_through_the_normalizer_and_raw():
    """"<|STARTOFTEXT|>" is matched behind the normalizer, "<|endoftext|>" raw -- "<|ENDOFTEXT|>" is text"""
    v = _v()
    tok = _tok()
    added = {a["content"]: a["id"] for a in json.loads(load_tokenizer_json(NAME))["added_tokens"]}
    docs = cc.added_docs() + cc.norm_docs()
    got = tok.encode_batch(docs, add_special_tokens=False)
    _hold_encodings(got, docs, v)
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v)
    assert list(got[1].ids) == [added[cc.SOT]] and list(got[5].ids) == [added[cc.EOT]] and added[cc.EOT] not in list(got[6].ids)
    with pytest.raises(ta.UnsupportedError, match="decode_batch: added token '<\\|startoftext\\|>' is normalized behind a normalizer"):
        tok.decode_batch([[added[cc.SOT], 5]])


def test_special_tokens_pairs_and_truncation_77_with_padding():
    v = _v()
    tok = _tok()
    s = v["special"]
    got = tok.encode_batch(s["docs"], add_special_tokens=True)
    for i in range(len(s["docs"])):
        assert list(got[i].ids) == s["ids"][i] and [tuple(o) for o in got[i].offsets] == _pairs(s["offsets_char"][i]) and list(got[i].word_ids) == s["words"][i], s["docs"][i]
        assert list(got[i].type_ids) == s["type_ids"][i] and list(got[i].special_tokens_mask) == s["special_tokens_mask"][i]
    p = v["pairs"]
    pairs = [tuple(x) for x in p["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    for i in range(len(pairs)):
        assert list(got[i].ids) == p["ids"][i] and list(got[i].type_ids) == p["type_ids"][i], pairs[i]
        assert [tuple(o) for o in got[i].offsets] == _pairs(p["offsets_char"][i]) and list(got[i].word_ids) == p["words"][i]
        assert list(got[i].special_tokens_mask) == p["special_tokens_mask"][i] and list(got[i].sequence_ids) == p["sequence_ids"][i]
    c = v["clip77"]
    tp = _tok()
    tp.enable_truncation(max_length=c["max_length"])
    tp.enable_padding(pad_id=c["pad_id"], pad_token=c["pad_token"], length=c["max_length"])
    got = tp.encode_batch(c["docs"], add_special_tokens=True)
    assert any(sum(m) == 77 for m in c["attention_mask"]) and any(sum(m) < 20 for m in c["attention_mask"])
    for i in range(len(c["docs"])):
        assert list(got[i].ids) == c["ids"][i] and len(got[i].ids) == 77, c["docs"][i]
        assert list(got[i].attention_mask) == c["attention_mask"][i] and list(got[i].special_tokens_mask) == c["special_tokens_mask"][i]
        assert [tuple(o) for o in got[i].offsets] == _pairs(c["offsets_char"][i]) and list(got[i].word_ids) == c["words"][i]


def test_decode_batch_of_the_variant_without_a_normalized_token():
    """pieces keep "</w>" literally, as the reference's ByteLevel decoder leaves them"""
    v = _v(PLAIN)
    tok = _tok(PLAIN)
    docs = v["docs"]
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v, what=PLAIN)
    ids = [v["ids"][i] for i in v["decode"]["index"]]
    assert tok.decode_batch(ids, skip_special_tokens=False) == v["decode"]["decoded"]
    assert tok.decode_batch(ids, skip_special_tokens=True) == v["decode"]["decoded_skip"]
    assert "the</w>" in v["decode"]["decoded"][docs.index("the the")]


def test_same_device_twice():
    v = _v()
    tok = _tok()
    two = ta.Tokenizer.from_str(load_tokenizer_json(NAME), device=[0, 0])
    docs = [d for d in v["docs"] if len(d) < 300] * 2
    a = tok.encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)


def test_live_differential_against_the_wheel(ref_tokenizers):
    """ids, offsets and word ids of 2,000 seeded documents of the probe's atoms against the wheel itself, and of the four accepted spellings"""
    docs = cc.random_docs(2000, seed=905) + cc.prompts(64, seed=906)
    exp = None
    for norm in ([cc.NFC, cc.REPLACE, cc.LOWER], [cc.NFC, cc.LOWER]):
        for use_regex in (True, False):
            js = cc.file_of(normalizer={"type": "Sequence", "normalizers": norm},
                            pre_tokenizer={"type": "Sequence", "pretokenizers": [cc.SPLIT, dict(cc.BYTELEVEL, use_regex=use_regex)]})
            if exp is None:
                exp = ref_tokenizers.Tokenizer.from_str(js).encode_batch(docs, add_special_tokens=True)
            got = ta.Tokenizer.from_str(js, device=0).encode_batch(docs, add_special_tokens=True)
            for k, x in enumerate(docs):
                assert list(got[k].ids) == exp[k].ids and [tuple(o) for o in got[k].offsets] == exp[k].offsets and list(got[k].word_ids) == exp[k].word_ids, (norm, use_regex, x)
