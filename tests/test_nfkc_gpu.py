"""The NFKC normalizer on the device (NORM_NFKC: kernels/nfkc.hip, the K mode of csrc/nfc_core.hpp) in front of the "▁" front and BPE over
characters or Unigram -- the layout the reference's SentencePieceBPETokenizer class builds: the wheel's vectors
(tools/make_golden_nfkc.py), every array, of documents built so that a char NFKC changes -- 3 bytes to 2, to 1, to a space the front must
split at, to 33 -- sits where the kernels can go wrong: ending at and straddling a 16-byte lane, a 64-byte word and a 4,096-byte
workgroup, first and last in a document; runs of hundreds of such chars that the widened head rule cuts; documents that are only marks;
marks behind a raw added-token match; the normalized added token.  Also the CPU rehearsal of all this under TKAMD_SIMT=1."""
import json

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import nfkc_cases as kc
from tests import unicode_chain_cases as uc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAMES = ["nfkc_spm_bpe", "nfkc_unigram"]
_VECTORS = {}


def _v(name):
    if name not in _VECTORS:
        _VECTORS[name] = load_vectors(name)
    return _VECTORS[name]


def _tok(name, **kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(name), device=0, **kw)


def _pairs(flat):
    return [(flat[2 * j], flat[2 * j + 1]) for j in range(len(flat) // 2)]


def _hold_csr(b, docs, v, idx, what=""):
    """ids, byte offsets, word ids of a CSR result against the vectors (idx: the documents' places in them)"""
    for k, d in enumerate(docs):
        i = idx[k]
        a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == v["ids"][i], (what, k, d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(v["offsets_char"][i])], (what, k, d[-24:])
        assert b.word_ids[a:z].tolist() == v["words"][i], (what, k, d[-24:])


@pytest.mark.parametrize("name", NAMES)
def test_vectors_every_array(name):
    """the whole batch at once: more than two workgroups of text, a document count that is no multiple of 256"""
    v = _v(name)
    tok = _tok(name)
    assert tok.info["normalizer"] == 6 and len(v["docs"]) % 256 and sum(len(d.encode("utf-8")) for d in v["docs"]) > 2 * 4096
    got = tok.encode_batch(v["docs"], add_special_tokens=False)
    for i, d in enumerate(v["docs"]):
        assert list(got[i].ids) == v["ids"][i], (name, d[-24:])
        assert [tuple(o) for o in got[i].offsets] == _pairs(v["offsets_char"][i]), (name, d[-24:])
        assert list(got[i].word_ids) == v["words"][i], (name, d[-24:])
    _hold_csr(tok.encode_batch_csr(v["docs"], offsets="byte", word_ids=True), v["docs"], v, range(len(v["docs"])), what=name)
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert [list(e.ids) for e in fast] == v["ids"]


@pytest.mark.parametrize("name", NAMES)
def test_changing_chars_at_lane_word_and_workgroup_edges(name):
    """each straddling document FIRST in its batch, so the char sits at exactly that byte of the text; and as the last bytes of one"""
    v = _v(name)
    tok = _tok(name)
    for d in kc.straddle_docs():
        docs = [d, "tail " + kc.FI]
        b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
        _hold_csr(b, docs[:1], v, [v["docs"].index(d)], what=(name, len(d)))


@pytest.mark.parametrize("name", NAMES)
def test_long_runs_are_cut_by_the_head_rule_and_not_refused(name):
    """200 fullwidth letters, 300 mixed fullwidth / ligature chars without a space, five U+FDFA in one lane (15 bytes become 165)"""
    v = _v(name)
    tok = _tok(name)
    docs = kc.long_run_docs()
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v, [v["docs"].index(d) for d in docs], what=name)
    for d in docs:                                         # ... and each first in a batch of its own
        _hold_csr(tok.encode_batch_csr([d, "x"], offsets="byte", word_ids=True), [d], v, [v["docs"].index(d)], what=(name, "alone"))


@pytest.mark.parametrize("name", NAMES)
def test_only_marks_empty_documents_and_chars_that_become_a_space(name):
    v = _v(name)
    tok = _tok(name)
    docs = kc.SPACE_DOCS
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    _hold_csr(b, docs, v, [v["docs"].index(d) for d in docs], what=name)
    assert int(b.tok_offsets[2]) == 0
    # "a U+3000 b": the front splits at the space U+3000 became -- two words
    k = docs.index("a" + kc.IDSP + "b")
    a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
    assert b.word_ids[a:z].tolist()[0] == 0 and b.word_ids[a:z].tolist()[-1] == 1
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0
    assert [len(e.ids) for e in tok.encode_batch(["", ""], add_special_tokens=False)] == [0, 0]


@pytest.mark.parametrize("name", NAMES)
def test_sixty_marks_are_refused_by_name_and_thirty_are_not(name):
    v = _v(name)
    tok = _tok(name)
    oks = ["A" + uc.MARKS30 + " b", kc.FW_A + uc.MARKS30 + kc.IDSP + "b"]
    got = tok.encode_batch(oks, add_special_tokens=False)
    for k, ok in enumerate(oks):
        assert list(got[k].ids) == v["ids"][v["docs"].index(ok)]
    for d in ("a" + uc.MARKS60, "x" * 50 + kc.FW_A + uc.MARKS60 + "y" * 50):
        with pytest.raises(ta.UnsupportedError, match="a character is followed by more than 48 combining characters"):
            tok.encode_batch(["fine", d, "fine too"], add_special_tokens=False)
    assert list(tok.encode_batch(oks[:1], add_special_tokens=False)[0].ids) == list(got[0].ids)      # (the handle goes on)


def test_added_tokens_raw_and_normalized():
    """a mark directly behind a raw match and at a document's start stays where it is; the composed, the fullwidth + decomposed and the
    all-fullwidth spelling all match the normalized token, and Encoding.tokens shows the match in its normalized form"""
    name = "nfkc_spm_bpe"
    v = _v(name)
    tok = _tok(name)
    added = {a["content"]: a["id"] for a in json.loads(load_tokenizer_json(name))["added_tokens"]}
    docs = kc.RAW_DOCS + kc.NORM_DOCS
    idx = [v["docs"].index(d) for d in docs]
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v, idx, what=name)
    got = tok.encode_batch(docs, add_special_tokens=True)
    for k, d in enumerate(docs):
        i = v["special"]["docs"].index(d)
        assert list(got[k].ids) == v["special"]["ids"][i] and list(got[k].tokens) == v["special"]["tokens"][i], d
        assert [list(o) for o in got[k].offsets] == v["special"]["offsets_char"][i], d
    assert added[kc.RAW_TOKEN] in got[0].ids and added[kc.NORM_TOKEN] in got[6].ids and "Caf\u00e9" in got[6].tokens
    assert added[kc.NORM_TOKEN] in got[7].ids and list(got[8].ids).count(added[kc.NORM_TOKEN]) == 2 and added[kc.NORM_TOKEN] in got[9].ids
    # the Metaspace decoder of the file is refused at the call; behind a decoder that is on the path the normalized added token is what
    # refuses it, as behind every normalizer
    with pytest.raises(ta.UnsupportedError, match="decode_batch: decoder type 'Metaspace' is outside the decode path"):
        tok.decode_batch([[added[kc.NORM_TOKEN]]])
    d = json.loads(load_tokenizer_json(name))
    d["decoder"] = json.loads(load_tokenizer_json("spm_bpe_llama2"))["decoder"]
    with pytest.raises(ta.UnsupportedError, match="decode_batch: added token '\uff23af\u00e9' is normalized behind a normalizer"):
        ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=0).decode_batch([[added[kc.NORM_TOKEN]]])


@pytest.mark.parametrize("token, char", [("\u0644", kc.SALLA), ("\u30f3", "\u3347")])
def test_a_normalized_token_that_occurs_several_times_in_one_chars_expansion(token, char, ref_tokenizers):
    """U+0644 occurs five times in what U+FDFA becomes, U+30F3 twice in U+3347's: more matches than the source text has bytes per
    shortest pattern.  The match list is bounded by the normalized text, and the result is the wheel's"""
    js = kc.file_of(added=[{"id": 10, "content": token, "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False}])
    w = ref_tokenizers.Tokenizer.from_str(js)
    tok = ta.Tokenizer.from_str(js, device=0)
    docs = [char * 6, char * 2, "a" + char * 40 + " b", char, "x " + token + char]
    for batch in ([docs[0]], docs):                        # (the first alone: 18 bytes of text, 30 matches)
        got = tok.encode_batch(batch, add_special_tokens=False)
        exp = w.encode_batch(batch, add_special_tokens=False)
        for k in range(len(batch)):
            assert list(got[k].ids) == exp[k].ids and [tuple(o) for o in got[k].offsets] == exp[k].offsets and list(got[k].word_ids) == exp[k].word_ids, (token, k)
    assert list(got[0].ids).count(10) == (30 if char == kc.SALLA else 12)


def test_raw_added_token_in_front_of_unigram():
    name = "nfkc_unigram"
    v = _v(name)
    tok = _tok(name)
    docs = kc.RAW_DOCS
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v, [v["docs"].index(d) for d in docs], what=name)
    got = tok.encode_batch(docs, add_special_tokens=True)
    for k, d in enumerate(docs):
        i = v["special"]["docs"].index(d)
        assert list(got[k].ids) == v["special"]["ids"][i] and list(got[k].tokens) == v["special"]["tokens"][i], d


@pytest.mark.parametrize("name", NAMES)
def test_template_pairs_truncation_overflow_pretokenized(name):
    v = _v(name)
    tok = _tok(name)
    s = v["special"]
    got = tok.encode_batch(s["docs"], add_special_tokens=True)
    for i in range(len(s["docs"])):
        assert list(got[i].ids) == s["ids"][i] and [list(o) for o in got[i].offsets] == s["offsets_char"][i] and list(got[i].word_ids) == s["words"][i]
        assert list(got[i].tokens) == s["tokens"][i]
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    for i in range(len(pairs)):
        assert list(got[i].ids) == v["pairs"]["ids"][i], pairs[i]
        assert list(got[i].type_ids) == v["pairs"]["type_ids"][i]
        assert [list(o) for o in got[i].offsets] == v["pairs"]["offsets_char"][i]
        assert list(got[i].word_ids) == v["pairs"]["words"][i]
    tp = _tok(name)
    tp.enable_truncation(max_length=v["trunc_pad"]["max_length"], stride=v["trunc_pad"]["stride"])
    tp.enable_padding(pad_id=v["trunc_pad"]["pad_id"], pad_token=v["trunc_pad"]["pad_token"])
    got = tp.encode_batch(s["docs"], add_special_tokens=True)
    for i in range(len(s["docs"])):
        assert list(got[i].ids) == v["trunc_pad"]["ids"][i] and list(got[i].attention_mask) == v["trunc_pad"]["attention_mask"][i]
        assert [list(o) for o in got[i].offsets] == v["trunc_pad"]["offsets_char"][i]
        assert [list(o.ids) for o in got[i].overflowing] == v["trunc_pad"]["overflowing_ids"][i]
    got = tok.encode_batch(v["pretok"]["inputs"], is_pretokenized=True, add_special_tokens=False)
    for i in range(len(v["pretok"]["inputs"])):
        assert list(got[i].ids) == v["pretok"]["ids"][i] and list(got[i].word_ids) == v["pretok"]["words"][i], v["pretok"]["inputs"][i]
        assert [list(o) for o in got[i].offsets] == v["pretok"]["offsets_char"][i]


@pytest.mark.parametrize("name", NAMES)
def test_mixed_batch_and_encode_packed(name):
    v = _v(name)
    tok = _tok(name)
    singles, pairs = v["special"], v["pairs"]
    inputs, want = [], []
    for k in range(12):
        inputs.append(singles["docs"][k])
        want.append(singles["ids"][k])
        inputs.append(tuple(pairs["inputs"][k]))
        want.append(pairs["ids"][k])
    got = tok.encode_batch(inputs, add_special_tokens=True)
    assert [list(e.ids) for e in got] == want
    docs = [d for d in v["docs"] if len(d) < 200]
    buf, off = ta.pack_documents(docs)
    b = tok.encode_packed(buf, off, "char", True)
    for k, d in enumerate(docs):
        i = v["docs"].index(d)
        a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
        assert b.ids[a:z].tolist() == v["ids"][i] and b.offsets[a:z].reshape(-1).tolist() == v["offsets_char"][i] and b.word_ids[a:z].tolist() == v["words"][i]


@pytest.mark.parametrize("name", NAMES)
def test_same_device_twice(name):
    v = _v(name)
    tok = _tok(name)
    two = ta.Tokenizer.from_str(load_tokenizer_json(name), device=[0, 0])
    docs = [d for d in v["docs"] if len(d) < 300] * 2
    a = tok.encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)


@pytest.mark.needs_hw
def test_device_entry():
    import torch
    name = "nfkc_spm_bpe"
    v = _v(name)
    buf, off = ta.pack_documents(v["docs"])
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    tok = _tok(name)
    for _ in range(2):
        b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(v["docs"]), int(off[-1]), stream=torch.cuda.current_stream().cuda_stream).sync()
        ids = b.ids_tensor().cpu().numpy().view("uint32")
        tof = b.tok_offsets_tensor().cpu().numpy()
        for i in range(len(v["docs"])):
            assert ids[tof[i]:tof[i + 1]].tolist() == v["ids"][i]


@pytest.mark.parametrize("name", NAMES)
def test_live_differential_against_the_wheel(name, ref_tokenizers):
    """ids, offsets, word ids and tokens of 600 seeded strings of bases, compatibility chars, marks and jamo against the wheel itself"""
    js = load_tokenizer_json(name)
    w = ref_tokenizers.Tokenizer.from_str(js)
    tok = ta.Tokenizer.from_str(js, device=0)
    docs = [" ".join(kc.seeded_strings(4, seed=900 + k)) for k in range(600)] + ["Hello, y'all! How are you \U0001f601 ?", "\uff28\u00e9llo\u3000\uff39'ALL \ufb01n"]
    got = tok.encode_batch(docs, add_special_tokens=True)
    exp = w.encode_batch(docs, add_special_tokens=True)
    for k, x in enumerate(docs):
        assert list(got[k].ids) == exp[k].ids and [tuple(o) for o in got[k].offsets] == exp[k].offsets and list(got[k].word_ids) == exp[k].word_ids, [hex(ord(c)) for c in x]
        assert list(got[k].tokens) == exp[k].tokens
