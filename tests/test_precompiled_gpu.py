"""Unigram behind the Precompiled normalizer on the device (kernels/precompiled.hip in front of the "▁" front): the XLM-R layout
(Sequence[Precompiled, Replace " {2,}"] + Sequence[WhitespaceSplit, Metaspace]) and Precompiled in front of bare Metaspace, against the
reference wheel's vectors (tools/make_golden_precompiled.py over tests/precompiled_cases.py) -- every array, through every entry -- and a
live differential where the wheel is importable.  Without the normalizer's path every test here fails at from_str."""
import json
import random

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import precompiled_cases as pc
from tests.helpers import char_to_byte, load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu
NAMES = pc.NAMES


@pytest.fixture(scope="module")
def vectors():
    return {n: load_vectors(n) for n in NAMES}


@pytest.fixture(scope="module")
def toks():
    return {n: ta.Tokenizer.from_str(load_tokenizer_json(n), device=0) for n in NAMES}


def _pairs(flat):
    return [[flat[2 * j], flat[2 * j + 1]] for j in range(len(flat) // 2)]


def _hold(name, e, v, i, d):
    assert list(e.ids) == v["ids"][i], (name, i, d[:40])
    assert [list(o) for o in e.offsets] == _pairs(v["offsets_char"][i]), (name, i, d[:40])
    assert list(e.word_ids) == v["words"][i], (name, i, d[:40])


def _hold_csr(name, b, v, idx, docs, unit):
    for k, i in enumerate(idx):
        a, z = int(b.tok_offsets[k]), int(b.tok_offsets[k + 1])
        assert b.ids[a:z].tolist() == v["ids"][i], (name, i, docs[k][:40])
        exp = _pairs(v["offsets_char"][i])
        if unit == "byte":
            m = char_to_byte(docs[k])
            exp = [[m[x], m[y]] for x, y in exp]
        assert b.offsets[a:z].tolist() == exp, (name, unit, i, docs[k][:40])
        assert b.word_ids[a:z].tolist() == v["words"][i], (name, i, docs[k][:40])


@pytest.mark.parametrize("name", NAMES)
def test_vectors_encode_batch(name, toks, vectors):
    v = vectors[name]
    got = toks[name].encode_batch(v["docs"], add_special_tokens=False)
    for i, d in enumerate(v["docs"]):
        _hold(name, got[i], v, i, d)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("unit", ["byte", "char"])
def test_vectors_csr_offsets_and_word_ids(name, unit, toks, vectors):
    v = vectors[name]
    b = toks[name].encode_batch_csr(v["docs"], offsets=unit, word_ids=True)
    _hold_csr(name, b, v, range(len(v["docs"])), v["docs"], unit)


@pytest.mark.parametrize("name", NAMES)
def test_vectors_fast_and_packed(name, toks, vectors):
    v = vectors[name]
    fast = toks[name].encode_batch_fast(v["docs"], add_special_tokens=False)
    buf, off = ta.pack_documents(v["docs"])
    p = toks[name].encode_packed(buf, off)
    for i, d in enumerate(v["docs"]):
        assert list(fast[i].ids) == v["ids"][i], (name, i, d[:40])
        assert p.ids[int(p.tok_offsets[i]):int(p.tok_offsets[i + 1])].tolist() == v["ids"][i], (name, i, d[:40])


@pytest.mark.parametrize("name", NAMES)
def test_every_edge_document_first_in_its_batch(name, toks, vectors):
    """the cluster sits at exactly the byte the document puts it at: behind 15 / 63 / 4,095 bytes, first, last, behind an added token"""
    v = vectors[name]
    edge = pc.edge_documents()
    assert v["docs"][:len(edge)] == edge
    rng = random.Random(5)
    for i, d in enumerate(edge):
        rest = rng.sample(range(len(edge)), 2)
        b = toks[name].encode_batch_csr([d] + [edge[r] for r in rest], offsets="char", word_ids=True)
        _hold_csr(name, b, v, [i] + rest, [d] + [edge[r] for r in rest], "char")


@pytest.mark.parametrize("name", NAMES)
def test_clusters_cut_by_a_document_edge_and_by_an_added_token(name, toks, vectors):
    """one document ends in a cluster's first char, the next begins with the rest (a mark, a ZWJ, an LF opens the piece); the same around <mask>"""
    v = vectors[name]
    where = {d: i for i, d in enumerate(v["docs"])}
    docs = []
    for a, b in pc.split_clusters():
        docs += ["x y" + a, b + " z", a + "<mask>" + b, "q" * 14 + a + "<mask>" + b]
    idx = [where[d] for d in docs]
    for unit in ("char", "byte"):
        _hold_csr(name, toks[name].encode_batch_csr(docs, offsets=unit, word_ids=True), v, idx, docs, unit)
    got = toks[name].encode_batch(docs[::-1], add_special_tokens=False)
    for k, d in enumerate(docs[::-1]):
        _hold(name, got[k], v, where[d], d)


@pytest.mark.parametrize("name", NAMES)
def test_the_batch_reversed(name, toks, vectors):
    v = vectors[name]
    n = len(v["docs"])
    docs = v["docs"][::-1]
    b = toks[name].encode_batch_csr(docs, offsets="byte", word_ids=True)
    _hold_csr(name, b, v, range(n - 1, -1, -1), docs, "byte")


@pytest.mark.parametrize("name", NAMES)
def test_template_pairs_truncation_padding(name, vectors):
    v = vectors[name]
    tok = ta.Tokenizer.from_str(load_tokenizer_json(name), device=0)
    got = tok.encode_batch(v["docs"], add_special_tokens=True)
    for i, d in enumerate(v["docs"]):
        _hold(name, got[i], v["special"], i, d)
    pairs = [tuple(p) for p in v["pairs"]["inputs"]]
    got = tok.encode_batch(pairs, add_special_tokens=True)
    for i in range(len(pairs)):
        _hold(name, got[i], v["pairs"], i, pairs[i][0])
        assert list(got[i].type_ids) == v["pairs"]["type_ids"][i]
    single = v["trunc"]["inputs"]
    tok.enable_truncation(max_length=v["trunc"]["max_length"], stride=v["trunc"]["stride"])
    got = tok.encode_batch_csr(single, add_special_tokens=True, overflowing=True)
    for i in range(len(single)):
        assert list(got[i].ids) == v["trunc"]["ids"][i]
        assert [list(o.ids) for o in got[i].overflowing] == v["trunc"]["overflowing"][i]
    tok.no_truncation()
    tok.enable_padding(pad_id=0, pad_token=v["pad"]["pad_token"])
    got = tok.encode_batch(single, add_special_tokens=True)
    for i in range(len(single)):
        assert list(got[i].ids) == v["pad"]["ids"][i]
        assert list(got[i].attention_mask) == v["pad"]["attention_mask"][i]


@pytest.mark.parametrize("name", NAMES)
def test_large_then_small_then_large_on_one_handle(name, toks, vectors):
    v = vectors[name]
    tok = toks[name]
    big = tok.encode_batch_csr(v["docs"], offsets="char", word_ids=True)
    small = tok.encode_batch_csr(v["docs"][:3], offsets="char", word_ids=True)
    _hold_csr(name, small, v, range(3), v["docs"][:3], "char")
    again = tok.encode_batch_csr(v["docs"], offsets="char", word_ids=True)
    for f in ("ids", "tok_offsets", "offsets", "word_ids"):
        assert np.array_equal(getattr(big, f), getattr(again, f)), f
    _hold_csr(name, again, v, range(len(v["docs"])), v["docs"], "char")


def _live_docs(seed):
    rng = random.Random(seed)
    pool = pc.clusters() + pc.table_rows() + ["a", "b", "ab", "xy", " ", "  ", "\t", "\n", pc.MS, "<s>", "</s>", "<mask>", " <mask> ", "\u4e2d\u6587", "\U0001f600", "caf\u00e9",
                                               "\uff21", "hello", "world", "q" * 17, "\u3000", "\u00a0", "\u2003", "\ufeff", "\u0301", "\u200d", "\u0e33", "\u094d", "\x1e"]
    return ["".join(rng.choice(pool) for _ in range(rng.randint(0, 24))) for _ in range(1500)] + [pc.prose(rng, rng.randint(10, 400), odd=0.15) for _ in range(150)]


def _hold_live(tok, w, docs):
    got = tok.encode_batch(docs, add_special_tokens=False)
    exp = w.encode_batch(docs, add_special_tokens=False)
    for k, d in enumerate(docs):
        assert list(got[k].ids) == exp[k].ids, d
        assert [tuple(o) for o in got[k].offsets] == exp[k].offsets, d
        assert list(got[k].word_ids) == exp[k].word_ids, d
    b = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    for k, d in enumerate(docs):
        m = char_to_byte(d)
        assert b.offsets[int(b.tok_offsets[k]):int(b.tok_offsets[k + 1])].tolist() == [[m[x], m[y]] for x, y in exp[k].offsets], d


@pytest.mark.parametrize("name", NAMES)
def test_live_differential(name, toks, ref_tokenizers):
    _hold_live(toks[name], ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name)), _live_docs(41 + NAMES.index(name)))


@pytest.mark.parametrize("scheme", ["first", "never"])
def test_live_differential_of_the_other_prepend_schemes_behind_bare_metaspace(scheme, ref_tokenizers):
    """MS_FIRST / MS_NEVER over the normalizer's text: a document start in normalized coordinates, behind chars that became nothing too"""
    d = json.loads(load_tokenizer_json("precompiled_ms"))
    d["pre_tokenizer"]["prepend_scheme"] = scheme
    js = json.dumps(d, ensure_ascii=False)
    docs = _live_docs(59) + ["\ufeffx y", "\x1e\x1e", "<mask>\ufeffx", "\ufeff<mask>x", " x", "\ufeff x", "\u200b\u2581x", "\t\x1ea"]
    _hold_live(ta.Tokenizer.from_str(js, device=0), ref_tokenizers.Tokenizer.from_str(js), docs)
