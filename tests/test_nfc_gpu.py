"""The NFC normalizer on the device (kernels/nfc.hip) in front of byte-level BPE: the wheel's vectors (tools/make_golden_nfc.py) of a
Qwen2-layout tokenizer and a GPT-2 ByteLevel one with trim_offsets -- every array -- and documents built so that a segment sits
where the kernels can go wrong: straddling a 16-byte lane, a 64-byte word and a 4,096-byte workgroup, first and last in a document,
across a document edge and an added-token match, the speculation and its pause, the refusal of a 60-mark segment; and a live
differential against the wheel where it imports.  Also the CPU rehearsal of all this under TKAMD_SIMT=1."""
import random

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import nfc_cases as nc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

NAMES = ["nfc_qwen2", "nfc_gpt2"]


def _tok(name, **kw):
    return ta.Tokenizer.from_str(load_tokenizer_json(name), device=0, **kw)


def _pairs(flat):
    return [(flat[2 * j], flat[2 * j + 1]) for j in range(len(flat) // 2)]


def _hold_csr(b, docs, v, idx=None, what=""):
    """ids, byte offsets, word ids of a CSR result against the vectors (idx: the documents' places in them)"""
    for k, d in enumerate(docs):
        i = k if idx is None else idx[k]
        a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
        m = char_to_byte(d)
        assert b.ids[a:z].tolist() == v["ids"][i], (what, k, d[-24:])
        assert [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in _pairs(v["offsets_char"][i])], (what, k, d[-24:])
        assert b.word_ids[a:z].tolist() == v["words"][i], (what, k, d[-24:])


@pytest.mark.parametrize("name", NAMES)
def test_vectors_every_array(name):
    v = load_vectors(name)
    tok = _tok(name)
    for _ in range(2):                                  # (the first batch speculates and is run again; the second normalizes outright)
        got = tok.encode_batch(v["docs"], add_special_tokens=False)
        for i, d in enumerate(v["docs"]):
            assert list(got[i].ids) == v["ids"][i], (name, d[-24:])
            assert [tuple(o) for o in got[i].offsets] == _pairs(v["offsets_char"][i]), (name, d[-24:])
            assert list(got[i].word_ids) == v["words"][i], (name, d[-24:])
    _hold_csr(tok.encode_batch_csr(v["docs"], offsets="byte", word_ids=True), v["docs"], v, what=name)
    fast = tok.encode_batch_fast(v["docs"], add_special_tokens=False)
    assert [list(e.ids) for e in fast] == v["ids"]


@pytest.mark.parametrize("name", NAMES)
def test_segments_at_lane_word_and_workgroup_edges(name):
    """each straddling document FIRST in its batch, so the segment sits at exactly that byte of the text; and as the last bytes of one"""
    v = load_vectors(name)
    tok = _tok(name)
    for d in nc.straddle_docs() + ["x" * 30 + nc.E, "x" * 4094 + nc.M3]:
        docs = [d, "tail e\u0301"]
        b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
        _hold_csr(b, docs[:1], v, [v["docs"].index(d)], what=(name, len(d)))


def test_a_char_that_straddles_from_a_copied_lane_into_a_walked_one(monkeypatch):
    """a three-byte char that is not active begins in the last byte(s) of a lane that is copied whole and ends in a lane that holds a
    mark: its tail is the walked lane's to write.  NFC text, so the file without the normalizer line says what must come out."""
    import json
    monkeypatch.setenv("TKAMD_TEST_HOOKS", "1")
    monkeypatch.setenv("TKAMD_NFC_SPEC", "0")           # (the normalizer's kernels outright, on a fresh handle)
    tok = _tok("nfc_qwen2")
    js = json.loads(load_tokenizer_json("nfc_qwen2"))
    js["normalizer"] = None
    plain = ta.Tokenizer.from_str(json.dumps(js, ensure_ascii=False), device=0)
    for k in (13, 14, 15, 16, 29, 30, 31, 63, 4095):
        docs = ["x " * (k // 2) + "x" * (k % 2) + nc.PROPER[0], nc.PROPER[1]]
        a = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
        b = plain.encode_batch_csr(docs, offsets="byte", word_ids=True)
        assert np.array_equal(a.ids, b.ids) and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids), k


@pytest.mark.parametrize("name", NAMES)
def test_a_mark_that_opens_a_piece_does_not_compose(name):
    v = load_vectors(name)
    tok = _tok(name)
    for docs in (["abce", "\u0301xyz"], ["abc\u1100", "\u1161\u11a8 x"], ["a<|endoftext|>\u0301b"], ["e<|im_start|>\u0301<|im_end|>e\u0301"]):
        idx = [v["docs"].index(x) for x in docs]
        _hold_csr(tok.encode_batch_csr(docs, offsets="byte", word_ids=True), docs, v, idx, what=name)
    # (composed, the pair would be one char less: "abc" + U+00E9 + "xyz")
    both = tok.encode_batch(["abce", "\u0301xyz", "abce\u0301xyz"], add_special_tokens=False)
    assert list(both[0].ids) + list(both[1].ids) != list(both[2].ids) and both[0].offsets[-1][1] == 4 and both[1].offsets[0] == (0, 1)


def test_normalized_added_token_written_decomposed():
    v = load_vectors("nfc_gpt2")
    tok = _tok("nfc_gpt2")
    vocab = {a["content"]: a["id"] for a in __import__("json").loads(load_tokenizer_json("nfc_gpt2"))["added_tokens"]}
    docs = ["caf\u00e9 au lait", "cafe\u0301 au lait", "xe\u0301e e\u0301 e"]
    got = tok.encode_batch(docs, add_special_tokens=False)
    for k, d in enumerate(docs):
        i = v["docs"].index(d)
        assert list(got[k].ids) == v["ids"][i] and [tuple(o) for o in got[k].offsets] == _pairs(v["offsets_char"][i]), d
    assert vocab["caf\u00e9 au"] in got[0].ids and vocab["caf\u00e9 au"] in got[1].ids and vocab["e\u0301e"] in got[2].ids


def test_proper_order_marks_do_not_leave_the_fast_path():
    """Thai tone marks, Devanagari virama, Arabic harakat, Hebrew points in canonical order are NFC and Quick_Check = Yes: the batch is
    not run again (the rerun counter stays), and the result is the vectors'"""
    v = load_vectors("nfc_qwen2")
    tok = _tok("nfc_qwen2")
    docs = nc.PROPER + ["plain ASCII text, nothing to do here at all", "caf\u00e9 na\u00efve r\u00e9sum\u00e9 Stra\u00dfe", "\ud55c\uad6d\uc5b4 \ubb38\uc7a5"]
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    _hold_csr(b, docs, v, [v["docs"].index(d) for d in docs])
    q = tok.queue_sizes()
    assert q["nfc_reruns"] == 0 and q["nfc_spec_pause"] == 0
    tok.encode_batch_csr(docs + ["e\u0301"])
    q = tok.queue_sizes()
    assert q["nfc_reruns"] == 1 and q["nfc_spec_pause"] > 0


def test_sixty_marks_are_refused_by_name_and_thirty_are_not():
    tok = _tok("nfc_qwen2")
    marks = "".join(chr(0x300 + (7 * k) % 0x30) for k in range(60))
    v = load_vectors("nfc_qwen2")
    ok = "a" + marks[:30] + " b"
    got = tok.encode_batch([ok], add_special_tokens=False)[0]
    assert list(got.ids) == v["ids"][v["docs"].index(ok)]
    for d in ("a" + marks, "x" * 50 + marks + "y" * 50):
        with pytest.raises(ta.UnsupportedError, match="NFC: a character is followed by more than 48 combining characters"):
            tok.encode_batch(["fine", d, "fine too"], add_special_tokens=False)
    assert list(tok.encode_batch([ok], add_special_tokens=False)[0].ids) == list(got.ids)      # (the handle goes on)


@pytest.mark.parametrize("name", NAMES)
def test_all_nfc_batch_is_the_same_with_and_without_speculation(name, monkeypatch):
    clean = [d for d in load_vectors(name)["docs"] if len(d) < 300 and all(ord(c) < 0x300 for c in d)] + nc.PROPER
    tok = _tok(name)
    a = tok.encode_batch_csr(clean, offsets="char", word_ids=True)
    assert tok.queue_sizes()["nfc_reruns"] == 0
    monkeypatch.setenv("TKAMD_TEST_HOOKS", "1")
    monkeypatch.setenv("TKAMD_NFC_SPEC", "0")           # never speculate (read when the handle is made): what TKAMD_NO_SPECULATION asks for per call
    b = _tok(name).encode_batch_csr(clean, offsets="char", word_ids=True)
    for x, y in ((a.ids, b.ids), (a.tok_offsets, b.tok_offsets), (a.offsets, b.offsets), (a.word_ids, b.word_ids)):
        assert np.array_equal(x, y)
    # ... and what the same file without the normalizer line computes (the parent's behaviour on such text)
    js = __import__("json").loads(load_tokenizer_json(name))
    js["normalizer"] = None
    c = ta.Tokenizer.from_str(__import__("json").dumps(js, ensure_ascii=False), device=0).encode_batch_csr(clean, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, c.ids) and np.array_equal(a.offsets, c.offsets) and np.array_equal(a.word_ids, c.word_ids)


@pytest.mark.parametrize("name", NAMES)
def test_no_speculation_flag_normalizes_outright(name):
    """TKAMD_NO_SPECULATION, the flag of a caller that never synchronises through the library: the normalizer's kernels run in the first
    and only run -- an all-NFC batch and one that is not are the vectors', and nothing is run again"""
    from tokenizers_amd import _lib
    v = load_vectors(name)
    tok = _tok(name)
    flags_of = tok._flags
    tok._flags = lambda *a: flags_of(*a) | _lib.NO_SPECULATION
    clean = [d for d in v["docs"] if len(d) < 300 and all(ord(c) < 0x300 for c in d)] + nc.PROPER
    dirty = [d for d in v["docs"] if len(d) < 300 and any(0x300 <= ord(c) < 0x370 for c in d)]
    assert len(clean) > 20 and len(dirty) > 20
    for docs in (clean, dirty, v["docs"]):
        b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
        _hold_csr(b, docs, v, [v["docs"].index(d) for d in docs], what=name)
        q = tok.queue_sizes()
        assert q["nfc_reruns"] == 0 and q["nfc_spec_pause"] == 0


def test_decode_of_normalized_added_tokens_stays_refused():
    with pytest.raises(ta.UnsupportedError, match="is normalized behind a normalizer"):
        _tok("nfc_gpt2").decode_batch([[1, 2, 3]], skip_special_tokens=False)
    assert _tok("nfc_qwen2").decode_batch([[]], skip_special_tokens=False) == [""]      # (normalized = false specials only: decodes)


def test_one_bad_document_among_63_and_the_batch_behind_it(ref_tokenizers):
    name = "nfc_qwen2"
    w = ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name))
    tok = _tok(name)
    from oracle import synth
    clean = synth.gen_lines(63, text_seed=81)
    docs = clean[:40] + ["the one e\u0301 document"] + clean[40:]
    for batch in (docs, clean):                         # (the second runs while the pause is in force: normalized outright)
        got = tok.encode_batch(batch, add_special_tokens=False)
        exp = w.encode_batch(batch, add_special_tokens=False)
        for k in range(len(batch)):
            assert list(got[k].ids) == exp[k].ids and [tuple(o) for o in got[k].offsets] == exp[k].offsets and list(got[k].word_ids) == exp[k].word_ids
    q = tok.queue_sizes()
    assert q["nfc_reruns"] == 1 and 0 < q["nfc_spec_pause"]


@pytest.mark.parametrize("name", NAMES)
def test_template_pairs_truncation_padding_pretokenized(name):
    v = load_vectors(name)
    tok = _tok(name)
    s = v["special"]
    got = tok.encode_batch(s["docs"], add_special_tokens=True)
    for i in range(len(s["docs"])):
        assert list(got[i].ids) == s["ids"][i] and [list(o) for o in got[i].offsets] == s["offsets_char"][i] and list(got[i].word_ids) == s["words"][i]
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    for i in range(len(pairs)):
        assert list(got[i].ids) == v["pairs"]["ids"][i], pairs[i]
        assert list(got[i].type_ids) == v["pairs"]["type_ids"][i]
        assert [list(o) for o in got[i].offsets] == v["pairs"]["offsets_char"][i]
        assert list(got[i].word_ids) == v["pairs"]["words"][i]
    tp = _tok(name)
    tp.enable_truncation(max_length=v["trunc_pad"]["max_length"], stride=v["trunc_pad"]["stride"])
    tp.enable_padding(pad_id=v["trunc_pad"]["pad_id"], pad_token="<|endoftext|>")
    got = tp.encode_batch(s["docs"], add_special_tokens=True)
    for i in range(len(s["docs"])):
        assert list(got[i].ids) == v["trunc_pad"]["ids"][i] and list(got[i].attention_mask) == v["trunc_pad"]["attention_mask"][i]
        assert [list(o) for o in got[i].offsets] == v["trunc_pad"]["offsets_char"][i]
    got = tok.encode_batch(v["pretok"]["inputs"], is_pretokenized=True, add_special_tokens=False)
    for i in range(len(v["pretok"]["inputs"])):
        assert list(got[i].ids) == v["pretok"]["ids"][i] and list(got[i].word_ids) == v["pretok"]["words"][i]
        assert [list(o) for o in got[i].offsets] == v["pretok"]["offsets_char"][i]


def test_empty_documents_and_empty_batch():
    tok = _tok("nfc_qwen2")
    b = tok.encode_batch_csr(["", "e\u0301", "", ""], offsets="byte", word_ids=True)
    assert b.tok_offsets.tolist()[0] == 0 and b.tok_offsets[1] == 0 and b.tok_offsets[2] == b.tok_offsets[4] > 0
    assert len(tok.encode_batch(["", ""], add_special_tokens=False)[0].ids) == 0
    assert len(tok.encode_batch([], add_special_tokens=False)) == 0


@pytest.mark.needs_hw
def test_device_entry():
    """synchronised (the first call is run again by sync()), then unsynced=True on a fresh handle: normalized in the one run"""
    import torch
    v = load_vectors("nfc_qwen2")
    buf, off = ta.pack_documents(v["docs"])
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def hold(b):
        ids = b.ids_tensor().cpu().numpy().view("uint32")
        tof = b.tok_offsets_tensor().cpu().numpy()
        for i in range(len(v["docs"])):
            assert ids[tof[i]:tof[i + 1]].tolist() == v["ids"][i]
    tok = _tok("nfc_qwen2")
    for _ in range(2):
        hold(tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(v["docs"]), int(off[-1]), stream=st).sync())
    assert tok.queue_sizes()["nfc_reruns"] == 1
    tok = _tok("nfc_qwen2")
    b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(v["docs"]), int(off[-1]), stream=st, unsynced=True)
    torch.cuda.synchronize()
    tof = b.tok_offsets_tensor().cpu().numpy()
    ids = b.ids_tensor_unsynced().cpu().numpy().view("uint32")      # (no sync(): the results as a stream-ordered consumer sees them)
    for i in range(len(v["docs"])):
        assert ids[tof[i]:tof[i + 1]].tolist() == v["ids"][i]
    assert tok.queue_sizes()["nfc_reruns"] == 0


def test_same_device_twice():
    v = load_vectors("nfc_gpt2")
    tok = _tok("nfc_gpt2")
    two = ta.Tokenizer.from_str(load_tokenizer_json("nfc_gpt2"), device=[0, 0])
    docs = v["docs"] * 2
    a = tok.encode_batch_csr(docs, offsets="char", word_ids=True)
    b = two.encode_batch_csr(docs, offsets="char", word_ids=True)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.tok_offsets, b.tok_offsets)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)


def _random_docs(rng, n):
    """<= 200 bytes each; the alphabet is half ASCII, half the active set and the bases it acts on"""
    active, _, _, _ = nc.tables()
    bases = nc.composing_starters()
    ascii_pool = list("abcdefghij  \n.,") + ["the ", "ing", "<|endoftext|>", "12"]
    out = []
    for _ in range(n):
        parts, size = [], 0
        for _ in range(rng.randint(0, 40)):
            c = rng.choice(ascii_pool) if rng.random() < 0.5 else chr(rng.choice(active) if rng.random() < 0.6 else rng.choice(bases))
            size += len(c.encode("utf-8"))
            if size > 200:
                break
            parts.append(c)
        out.append("".join(parts))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_live_differential(name, ref_tokenizers):
    w = ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name))
    tok = _tok(name)
    docs = _random_docs(random.Random(91 + NAMES.index(name)), 2000)
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    bad = 0
    for k, d in enumerate(docs):
        m = char_to_byte(d)
        a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
        ok = (list(got[k].ids) == exp[k].ids and [tuple(o) for o in got[k].offsets] == exp[k].offsets and list(got[k].word_ids) == exp[k].word_ids and
              [tuple(o) for o in b.offsets[a:z].tolist()] == [(m[x], m[y]) for x, y in exp[k].offsets])
        bad += not ok
        assert ok, [hex(ord(c)) for c in d]
    assert bad == 0
