#!/usr/bin/env python3
"""Golden fixtures for Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family, written with the REFERENCE wheel:
    digits_individual   Sequence[Digits(individual_digits=true), ByteLevel(add_prefix_space=false, use_regex=true)]
    digits_contiguous   the same with individual_digits=false
both with no normalizer, a ByteLevel decoder, a TemplateProcessing with the BOS token in front and added tokens special and not, over the
vocabulary and merges of tests/golden/split_qwen2.json.gz.  tests/golden/<name>.json.gz and <name>_vectors.json.gz: ids, char offsets
(flat pairs; the byte offsets follow from them and the text) and word ids of tests/digits_cases.py edge_docs() -- every one encoded alone,
at byte 0 of its batch -- of its batches() and of some prose; the decoded strings; one 70 KB document.  digits_individual also: the same
with the special tokens (type ids, special-tokens masks); pairs; pre-tokenized input; encode_special_tokens; truncation with a stride and
what it cuts off; padding of both kinds; NFC in front.  Runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from oracle import synth  # noqa: E402
from tests import digits_cases as dc  # noqa: E402
from tests.helpers import load_tokenizer_json  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
# (decomposed: NFC changes them, so a batch that holds one goes through the normalizer's general path)
NFC_DOCS = ["cafe\u0301 12", "plain 34 text", "1a\u030a2", "x" * 62 + "e\u0301" + "7", "\u0663a\u0308\u0664", "no change 5"]


def layout(individual):
    d = json.loads(load_tokenizer_json("split_qwen2"))
    nxt = max(d["model"]["vocab"].values()) + 1
    added = [(dc.BOS, True), (dc.EOS, True), (dc.PAD, True), (dc.USER, False), (dc.ASSISTANT, False)]
    d["added_tokens"] = [{"id": nxt + k, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": s}
                         for k, (c, s) in enumerate(added)]
    d["normalizer"] = None
    d["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [
        {"type": "Digits", "individual_digits": individual},
        {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}]}
    d["decoder"] = {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True}
    d["post_processor"] = {
        "type": "TemplateProcessing",
        "single": [{"SpecialToken": {"id": dc.BOS, "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}],
        "pair": [{"SpecialToken": {"id": dc.BOS, "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                 {"SpecialToken": {"id": dc.BOS, "type_id": 1}}, {"Sequence": {"id": "B", "type_id": 1}}],
        "special_tokens": {dc.BOS: {"id": dc.BOS, "ids": [nxt], "tokens": [dc.BOS]}}}
    return json.dumps(d, ensure_ascii=False), nxt + 2


def flat(e):
    return [x for o in e.offsets for x in o]


def arrays(encs):
    return {"ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs]}


def emit(name, individual):
    js, pad_id = layout(individual)
    tok = Tokenizer.from_str(js)
    edge = dc.edge_docs()
    # every edge document alone: at byte 0 of its batch, as the tests encode it
    v = {"reference": f"tokenizers=={tokenizers.__version__}", "edge": arrays([tok.encode(d, add_special_tokens=False) for d in edge])}
    v["batches"] = [arrays(tok.encode_batch(b, add_special_tokens=False)) for b in dc.batches()]
    dd = [d for d in edge if len(d) < 400] + synth.gen_lines(40, text_seed=81) + dc.random_strings(40, seed=82, lo=10, hi=90, alphabet=dc.WIDE)
    v["docs"] = dd
    v.update(arrays(tok.encode_batch(dd, add_special_tokens=False)))
    v["decoded"] = tok.decode_batch(v["ids"], skip_special_tokens=False)
    v["decoded_skip"] = tok.decode_batch(v["ids"], skip_special_tokens=True)
    big = dc.big_doc()
    v["big"] = dict(arrays([tok.encode(big, add_special_tokens=False)]), n_bytes=len(big.encode("utf-8")))
    if individual:
        encs = tok.encode_batch(dd, add_special_tokens=True)
        v["special"] = dict(arrays(encs), type_ids=[e.type_ids for e in encs], special_tokens_mask=[e.special_tokens_mask for e in encs])
        small = [d for d in dd if len(d) < 120]
        pairs = [(small[i], small[(i * 7 + 3) % len(small)]) for i in range(0, len(small), 2)]
        encs = tok.encode_batch(pairs, add_special_tokens=True)
        v["pairs"] = dict(arrays(encs), inputs=[list(p) for p in pairs], type_ids=[e.type_ids for e in encs],
                          special_tokens_mask=[e.special_tokens_mask for e in encs], sequence_ids=[e.sequence_ids for e in encs])
        t2 = Tokenizer.from_str(js)
        t2.encode_special_tokens = True
        v["encode_special"] = arrays(t2.encode_batch(dd, add_special_tokens=False))
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
        t4.enable_padding(pad_id=pad_id, pad_token=dc.PAD)
        encs = t4.encode_batch(small, add_special_tokens=True)
        v["pad"] = {"pad_id": pad_id, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs], "offsets_char": [flat(e) for e in encs]}
        t5 = Tokenizer.from_str(js)
        t5.enable_truncation(max_length=12)
        t5.enable_padding(pad_id=pad_id, pad_token=dc.PAD, length=12, direction="left")
        encs = t5.encode_batch(small, add_special_tokens=True)
        v["pad_fixed_left"] = {"length": 12, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs],
                               "special_tokens_mask": [e.special_tokens_mask for e in encs]}
        words_in = [["a  1", "x=12"], ["1", "2", "34"], ["12345", "  ", "it's 3pm"], ["plain", "words"], [""], ["1" * 70, " " * 70 + "7"], [dc.USER + "1", "b2"], ["٣٤", "Ⅷ½"]]
        v["pretok"] = dict(arrays(tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)), inputs=words_in)
        d6 = json.loads(js)
        d6["normalizer"] = {"type": "NFC"}
        t6 = Tokenizer.from_str(json.dumps(d6, ensure_ascii=False))
        v["nfc"] = dict(arrays(t6.encode_batch(NFC_DOCS, add_special_tokens=False)), docs=NFC_DOCS)
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    emit("digits_individual", True)
    emit("digits_contiguous", False)
