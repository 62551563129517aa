"""The Gemma-2 / Gemma-3 layout: normalizer Replace(" " -> "▁") (or Prepend + Replace) in front of the pre-tokenizer
Split(String " ", MergedWithPrevious, invert=false).  Behind that normalizer no space is left to split at, so the Split is inert and the
file loads as the "▁" front (PT_METASPACE) exactly as the same file with pre_tokenizer null does.  Here: the load, by kind; the encoding
on the host build of the kernels (the SIMT emulation, as tests/test_launch_sequence.py opens it) against the null layout, array by array,
and against the reference wheel reading the Split itself; and the refusals of everything near it, by name.  No real Gemma file is among the
fixtures: the two "▁" fixtures carry the Split in place of their null pre-tokenizer, and a real Gemma vocabulary loads only if it
passes the whole-piece checks (the crossing-merge proof) these fixtures pass."""
import json
import random

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import test_launch_sequence as base
from tests.helpers import load_tokenizer_json, load_vectors

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

NAMES = ["spm_bpe_llama2", "spm_bpe_replace_only"]
GEMMA_SPLIT = {"type": "Split", "pattern": {"String": " "}, "behavior": "MergedWithPrevious", "invert": False}


def _js(name, pre=GEMMA_SPLIT, **over):
    d = json.loads(load_tokenizer_json(name))
    assert d["pre_tokenizer"] is None
    d["pre_tokenizer"] = pre
    d.update(over)
    return json.dumps(d, ensure_ascii=False)


def _docs(name):
    rng = random.Random(7)
    alphabet = ["a", "b", "hello", "world", " ", " ", "  ", "\t", "\n", "▁", "é", "中", "\U0001F600", "<s>", "</s>", "<unk>", ".", "▁ ", " ▁"]
    return load_vectors(name)["docs"] + ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 30))) for _ in range(300)] + ["", " ", "  ", "▁", " a ", "a  b"]


@pytest.mark.parametrize("name", NAMES)
def test_loads_as_the_bar_front(name):
    info = ta.Tokenizer.from_str(_js(name), device=-1).info
    assert info["pre_tokenizer"] == 7 and info["normalizer"] == 2
    null = ta.Tokenizer.from_str(load_tokenizer_json(name), device=-1).info
    assert {k: v for k, v in info.items()} == {k: v for k, v in null.items()}
    # (invert defaults to false)
    assert ta.Tokenizer.from_str(_js(name, pre={k: v for k, v in GEMMA_SPLIT.items() if k != "invert"}), device=-1).info["pre_tokenizer"] == 7


@pytest.mark.parametrize("name", NAMES)
def test_encodes_as_the_null_layout_and_as_the_wheel(name, ref_tokenizers):
    docs = _docs(name)
    ours = ta.Tokenizer.from_str(_js(name), device=0)
    null = ta.Tokenizer.from_str(load_tokenizer_json(name), device=0)
    for mode in ("char", "byte"):
        a = ours.encode_batch_csr(docs, offsets=mode, word_ids=True)
        b = null.encode_batch_csr(docs, offsets=mode, word_ids=True)
        assert np.array_equal(a.tok_offsets, b.tok_offsets) and np.array_equal(a.ids, b.ids)
        assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.word_ids, b.word_ids)
    wheel = ref_tokenizers.Tokenizer.from_str(_js(name))
    exp = wheel.encode_batch(docs, add_special_tokens=False)
    got = ours.encode_batch(docs, add_special_tokens=False)
    for i, d in enumerate(docs):
        assert list(got[i].ids) == exp[i].ids, (name, d)
        assert [tuple(o) for o in got[i].offsets] == exp[i].offsets, (name, d)
        assert list(got[i].word_ids) == exp[i].word_ids, (name, d)


REFUSED = [
    (dict(GEMMA_SPLIT, invert=True), "Split\\(String ' '\\) with invert = true behind the U\\+2581 normalizers"),
    (dict(GEMMA_SPLIT, pattern={"String": "\t"}), "Split with the String pattern '\t' behind the U\\+2581 normalizers"),
    (dict(GEMMA_SPLIT, pattern={"String": "  "}), "Split with the String pattern '  ' behind the U\\+2581 normalizers"),
    (dict(GEMMA_SPLIT, pattern={"Regex": " "}), "Split with a Regex pattern behind the U\\+2581 normalizers"),
    (dict(GEMMA_SPLIT, behavior="Isolated"), "Split\\(String ' '\\) with behavior 'Isolated' behind the U\\+2581 normalizers"),
    (dict(GEMMA_SPLIT, behavior="Removed"), "Split\\(String ' '\\) with behavior 'Removed' behind the U\\+2581 normalizers"),
    (dict(GEMMA_SPLIT, behavior="MergedWithNext"), "Split\\(String ' '\\) with behavior 'MergedWithNext'"),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_everything_near_it_is_refused_by_name(name, k):
    pre, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        ta.Tokenizer.from_str(_js(name, pre=pre), device=-1)


@pytest.mark.parametrize("name", NAMES)
def test_the_split_without_the_normalizer_is_refused(name):
    with pytest.raises(ta.UnsupportedError, match="pre_tokenizer: Split alone is outside the hot path"):
        ta.Tokenizer.from_str(_js(name, normalizer=None), device=-1)


def test_the_whole_piece_checks_stay_in_force():
    """what the null layout refuses of the model, the Split layout refuses with the same words"""
    for edit, msg in ((lambda d: d["model"].__setitem__("ignore_merges", True), "ignore_merges"),
                      (lambda d: d["model"].__setitem__("end_of_word_suffix", "</w>") or d["model"].__setitem__("byte_fallback", False), "end_of_word_suffix")):
        for pre in (None, GEMMA_SPLIT):
            d = json.loads(load_tokenizer_json("spm_bpe_llama2"))
            d["pre_tokenizer"] = pre
            edit(d)
            with pytest.raises(ta.UnsupportedError, match=msg):
                ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=-1)
