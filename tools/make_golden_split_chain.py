#!/usr/bin/env python3
"""Golden fixtures for the chained Split pre-tokenizer of DeepSeek-V3 / R1, written with the REFERENCE wheel:
    ds3_chain   normalizer Sequence[], Sequence[Split(\\p{N}{1,3}), Split(CJK class +), Split(main pattern), ByteLevel(use_regex=false)], a
                ByteLevel decoder, a TemplateProcessing with the BOS token in front, added tokens in the DeepSeek style (special and not)
over the vocabulary and merges of tests/golden/split_qwen2.json.gz.  tests/golden/ds3_chain.json.gz and ds3_chain_vectors.json.gz: ids,
char offsets (flat pairs; the byte offsets follow from them and the text), word ids of tests/split_chain_cases.py edge_docs() and some
prose; the same with the special tokens (type ids, special-tokens masks); pairs; pre-tokenized input; truncation with a stride and what it
cuts off; padding of both kinds; the decoded strings; one 70 KB document and a batch of 300 short ones (ids only: the documents are
rebuilt by tests/split_chain_cases.py).  Runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from oracle import synth  # noqa: E402
from tests import split_chain_cases as sc  # noqa: E402
from tests.helpers import load_tokenizer_json  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "ds3_chain"

PRETOK = {"type": "Sequence", "pretokenizers": [
    {"type": "Split", "pattern": {"Regex": "\\p{N}{1,3}"}, "behavior": "Isolated", "invert": False},
    {"type": "Split", "pattern": {"Regex": "[一-龥぀-ゟ゠-ヿ]+"}, "behavior": "Isolated", "invert": False},
    {"type": "Split", "pattern": {"Regex": "[!\"#$%&'()*+,\\-./:;<=>?@\\[\\\\\\]^_`{|}~][A-Za-z]+|[^\r\n\\p{L}\\p{P}\\p{S}]?[\\p{L}\\p{M}]+| ?[\\p{P}\\p{S}]+[\r\n]*|"
                                           "\\s*[\r\n]+|\\s+(?!\\S)|\\s+"}, "behavior": "Isolated", "invert": False},
    {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}]}


def layout():
    d = json.loads(load_tokenizer_json("split_qwen2"))
    nxt = max(d["model"]["vocab"].values()) + 1
    added = [(sc.BOS, True), (sc.EOS, True), (sc.PAD, True), (sc.USER, False), (sc.ASSISTANT, False)]
    d["added_tokens"] = [{"id": nxt + k, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": s}
                         for k, (c, s) in enumerate(added)]
    d["normalizer"] = {"type": "Sequence", "normalizers": []}
    d["pre_tokenizer"] = PRETOK
    d["decoder"] = {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True}
    d["post_processor"] = {
        "type": "TemplateProcessing",
        "single": [{"SpecialToken": {"id": sc.BOS, "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}],
        "pair": [{"SpecialToken": {"id": sc.BOS, "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                 {"SpecialToken": {"id": sc.BOS, "type_id": 1}}, {"Sequence": {"id": "B", "type_id": 1}}],
        "special_tokens": {sc.BOS: {"id": sc.BOS, "ids": [nxt], "tokens": [sc.BOS]}}}
    return json.dumps(d, ensure_ascii=False), nxt + 2


def flat(e):
    return [x for o in e.offsets for x in o]


def emit():
    js, pad_id = layout()
    tok = Tokenizer.from_str(js)
    dd = sc.edge_docs() + synth.gen_lines(40, text_seed=71) + sc.random_strings(40, seed=72, lo=10, hi=90, alphabet=sc.WIDE)
    v = {"docs": dd, "reference": f"tokenizers=={tokenizers.__version__}"}
    encs = tok.encode_batch(dd, add_special_tokens=False)
    v.update({"ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs]})
    v["decoded"] = tok.decode_batch(v["ids"], skip_special_tokens=False)
    v["decoded_skip"] = tok.decode_batch(v["ids"], skip_special_tokens=True)
    encs = tok.encode_batch(dd, add_special_tokens=True)
    v["special"] = {"ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs],
                    "type_ids": [e.type_ids for e in encs], "special_tokens_mask": [e.special_tokens_mask for e in encs]}
    small = [d for d in dd if len(d) < 120]
    pairs = [(small[i], small[(i * 7 + 3) % len(small)]) for i in range(0, len(small), 2)]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = {"inputs": [list(p) for p in pairs], "ids": [e.ids for e in encs], "type_ids": [e.type_ids for e in encs],
                  "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs],
                  "special_tokens_mask": [e.special_tokens_mask for e in encs], "sequence_ids": [e.sequence_ids for e in encs]}
    t2 = Tokenizer.from_str(js)
    t2.encode_special_tokens = True
    encs = t2.encode_batch(dd, add_special_tokens=False)
    v["encode_special"] = {"ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs]}
    t3 = Tokenizer.from_str(js)
    t3.enable_truncation(max_length=9, stride=2)
    encs = t3.encode_batch(dd, add_special_tokens=True)
    v["trunc"] = {"max_length": 9, "stride": 2, "ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs],
                  "overflowing": [[o.ids for o in e.overflowing] for e in encs],
                  "overflowing_offsets_char": [[flat(o) for o in e.overflowing] for e in encs]}
    encs = t3.encode_batch(pairs, add_special_tokens=True)
    v["trunc"]["pair_ids"] = [e.ids for e in encs]
    v["trunc"]["pair_overflowing"] = [[o.ids for o in e.overflowing] for e in encs]
    t4 = Tokenizer.from_str(js)
    t4.enable_padding(pad_id=pad_id, pad_token=sc.PAD)
    encs = t4.encode_batch(small, add_special_tokens=True)
    v["pad"] = {"pad_id": pad_id, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs], "offsets_char": [flat(e) for e in encs]}
    t5 = Tokenizer.from_str(js)
    t5.enable_truncation(max_length=12)
    t5.enable_padding(pad_id=pad_id, pad_token=sc.PAD, length=12, direction="left")
    encs = t5.encode_batch(small, add_special_tokens=True)
    v["pad_fixed_left"] = {"length": 12, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs],
                           "special_tokens_mask": [e.special_tokens_mask for e in encs]}
    words_in = [["a  1", "中文abc"], ["x", ".b", "..b"], ["12345", "  ", "\x01\x02c"], ["plain", "words"], [""], ["1" * 70, " " * 70 + "x"], [sc.USER + "a", "b"]]
    encs = tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)
    v["pretok"] = {"inputs": words_in, "ids": [e.ids for e in encs], "words": [e.word_ids for e in encs], "offsets_char": [flat(e) for e in encs]}
    big = sc.big_doc()
    e = tok.encode(big, add_special_tokens=False)
    v["big"] = {"n_bytes": len(big.encode("utf-8")), "ids": e.ids, "offsets_char": flat(e), "words": e.word_ids}
    for key, docs in (("short_batch", sc.short_batch()), ("plain_batch", sc.plain_batch())):
        v[key] = {"ids": [e.ids for e in tok.encode_batch(docs, add_special_tokens=False)]}
    for fn, text in ((NAME + ".json.gz", js), (NAME + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    emit()
