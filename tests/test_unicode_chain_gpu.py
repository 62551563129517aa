"""The NFD / Lowercase / StripAccents normalizer chains on the device (NORM_CHAIN: kernels/bert_norm.hip over the chain's own tables; where
NFD stays visible, kernels/nfc.hip in its NFD mode) in front of WordPiece, WordLevel and BPE over characters: the wheel's vectors (tools/make_golden_unicode_chain.py) -- every array -- of
documents built so that a char which changes length sits where the kernels can go wrong: ending at and straddling a 16-byte lane, a
64-byte word and a 4,096-byte workgroup, first and last in a document; documents and words that normalize to nothing; marks behind a
raw added-token match; the normalized added token.  Also the CPU rehearsal of all this under TKAMD_SIMT=1."""
import json

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import unicode_chain_cases as uc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAMES = ["chain_nls_wp", "chain_l_wl", "chain_sl_bpe", "chain_nl_wp"]
STRIPS = ("chain_nls_wp", "chain_sl_bpe")               # StripAccents is a member: a mark alone leaves nothing
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
    assert tok.info["normalizer"] == 5 and len(v["docs"]) % 256
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
    for d in uc.straddle_docs(uc.CHANGING, uc.BIG):
        docs = [d, "tail \u00e9"]
        b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
        _hold_csr(b, docs[:1], v, [v["docs"].index(d)], what=(name, len(d)))


@pytest.mark.parametrize("name", NAMES)
def test_text_that_normalizes_to_nothing(name):
    v = _v(name)
    tok = _tok(name)
    docs = ["", "\u0301", "\u0301\u0488", "\u00c1B \u0301 \u00c1b", "a \u0301\u0316 b", "\u0301 x", "x \u0301"]
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    _hold_csr(b, docs, v, [v["docs"].index(d) for d in docs], what=name)
    assert int(b.tok_offsets[1]) == 0
    if name in STRIPS:                                  # (a mark alone leaves no token, the word ids go on counting)
        assert int(b.tok_offsets[3]) == 0
        a, z = int(b.tok_offsets[3]), int(b.tok_offsets[4])
        if name == "chain_nls_wp":
            assert b.word_ids[a:z].tolist() == [0, 0, 1, 1]
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0
    assert [len(e.ids) for e in tok.encode_batch(["", ""], add_special_tokens=False)] == [0, 0]


def test_nfd_visible_segments_at_the_edges_and_marks_out_of_order():
    """Sequence[NFD, Lowercase]: the NFC tests' straddling segments, each first in its batch; marks out of canonical order with their
    by-position offsets; a mark behind a raw added-token match and at a document's start neither moves nor joins across the edge"""
    from tests import nfc_cases as nc
    name = "chain_nl_wp"
    v = _v(name)
    tok = _tok(name)
    for d in nc.straddle_docs():
        docs = [d, "tail e\u0301"]
        _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs[:1], v, [v["docs"].index(d)], what=(name, len(d)))
    docs = uc.out_of_order_docs() + [uc.RAW_TOKEN + "\u0301 x", "a" + uc.RAW_TOKEN + "\u0301", "\u0301" + uc.RAW_TOKEN, "E\u0301" + uc.RAW_TOKEN + "\u0316\u0301e"]
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    _hold_csr(b, docs, v, [v["docs"].index(d) for d in docs], what=name)
    got = tok.encode_batch(docs, add_special_tokens=False)
    for k, d in enumerate(docs):
        assert [tuple(o) for o in got[k].offsets] == _pairs(v["offsets_char"][v["docs"].index(d)]), d
    # "e U+0301 U+0316" is ordered to e U+0316 U+0301, the offsets stay those of the source positions
    assert [tuple(o) for o in got[0].offsets][:3] == [(0, 1), (1, 2), (2, 3)] and len({tuple(o) for o in got[0].offsets[:3]}) == 3


def test_sixty_marks_are_refused_by_name_and_thirty_are_not():
    name = "chain_nl_wp"
    v = _v(name)
    tok = _tok(name)
    ok = "A" + uc.MARKS30 + " b"
    got = tok.encode_batch([ok], add_special_tokens=False)[0]
    assert list(got.ids) == v["ids"][v["docs"].index(ok)]
    for d in ("a" + uc.MARKS60, "x" * 50 + uc.MARKS60 + "y" * 50):
        with pytest.raises(ta.UnsupportedError, match="a character is followed by more than 48 combining characters"):
            tok.encode_batch(["fine", d, "fine too"], add_special_tokens=False)
    assert list(tok.encode_batch([ok], add_special_tokens=False)[0].ids) == list(got.ids)      # (the handle goes on)


def test_added_tokens_raw_and_normalized():
    """a mark directly behind a raw match and at a document's start stays where it is; CAF\u00c9 matches the normalized token Caf\u00e9, and
    Encoding.tokens shows the match in its normalized form"""
    name = "chain_sl_bpe"
    v = _v(name)
    tok = _tok(name)
    added = {a["content"]: a["id"] for a in json.loads(load_tokenizer_json(name))["added_tokens"]}
    docs = [uc.RAW_TOKEN + "\u0301 x", "a" + uc.RAW_TOKEN + "\u0301", "\u0301" + uc.RAW_TOKEN, "E\u0301" + uc.RAW_TOKEN + "\u0316\u0301e",
            "CAF\u00c9 au lait", "a caf\u00e9 b", "Cafe\u0301 CAFE\u0301", "xCaf\u00c9x"]
    idx = [v["docs"].index(d) for d in docs]
    _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v, idx, what=name)
    got = tok.encode_batch(docs, add_special_tokens=True)
    for k, d in enumerate(docs):
        i = v["special"]["docs"].index(d)
        assert list(got[k].ids) == v["special"]["ids"][i] and list(got[k].tokens) == v["special"]["tokens"][i], d
    assert added[uc.RAW_TOKEN] in got[0].ids and added[uc.NORM_TOKEN] in got[4].ids and "caf\u00e9" in got[4].tokens
    assert added[uc.NORM_TOKEN] in got[5].ids and added[uc.NORM_TOKEN] in got[7].ids


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
        assert list(got[i].ids) == v["pretok"]["ids"][i] and list(got[i].word_ids) == v["pretok"]["words"][i]
        assert [list(o) for o in got[i].offsets] == v["pretok"]["offsets_char"][i]


def test_mixed_batch_and_encode_packed():
    name = "chain_nls_wp"
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
    name = "chain_nls_wp"
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


def test_live_differential_of_the_quicktour_layout(ref_tokenizers):
    """Sequence[NFD, Lowercase, StripAccents] + Whitespace + BPE over characters with [UNK] + a [CLS] A [SEP] template, the file the
    reference's quicktour builds: ids, offsets, word ids of seeded strings of bases and marks against the wheel itself"""
    d = json.loads(load_tokenizer_json("bpe_ws_unk"))
    d["normalizer"] = uc.sequence("NLS")
    n = len(d["model"]["vocab"])
    d["added_tokens"] += [{"id": n + k, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}
                          for k, c in enumerate(("[CLS]", "[SEP]"))]
    d["post_processor"] = {"type": "TemplateProcessing",
                           "single": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}}],
                           "pair": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}},
                                    {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
                           "special_tokens": {c: {"id": c, "ids": [n + k], "tokens": [c]} for k, c in enumerate(("[CLS]", "[SEP]"))}}
    js = json.dumps(d, ensure_ascii=False)
    w = ref_tokenizers.Tokenizer.from_str(js)
    tok = ta.Tokenizer.from_str(js, device=0)
    docs = [" ".join(uc.seeded_strings(4, seed=500 + k)) for k in range(600)] + ["Hello, y'all! How are you \U0001f601 ?", "H\u00e9llo Y'ALL \u0130stanbul"]
    got = tok.encode_batch(docs, add_special_tokens=True)
    exp = w.encode_batch(docs, add_special_tokens=True)
    for k, x in enumerate(docs):
        assert list(got[k].ids) == exp[k].ids and [tuple(o) for o in got[k].offsets] == exp[k].offsets and list(got[k].word_ids) == exp[k].word_ids, [hex(ord(c)) for c in x]
        assert list(got[k].tokens) == exp[k].tokens
