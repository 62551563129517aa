#!/usr/bin/env python3
"""Golden fixtures for the BLOOM / BLOOMZ layout, written with the REFERENCE wheel:
    bloom_bpe   Sequence[Split(Regex " ?[^(\\s|[.,!?…。，、।۔،])]+", Isolated), ByteLevel(add_prefix_space=false, use_regex=false)]
with no normalizer, a ByteLevel(trim_offsets=false) post-processor, a ByteLevel decoder and added tokens special and not, over the
vocabulary and merges of tests/golden/split_qwen2.json.gz.  tests/golden/bloom_bpe.json.gz and bloom_bpe_vectors.json.gz: ids, char offsets
(flat pairs; the byte offsets follow from them and the text) and word ids of tests/bloom_cases.py short_docs(), some prose and random
strings, encoded as one batch; of its batches(); of its device_edge_docs(), every one encoded alone; the decoded strings; pairs;
pre-tokenized input; encode_special_tokens; truncation with a stride and what it cuts off; padding of both kinds; one 70 KB document.
Runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from oracle import synth  # noqa: E402
from tests import bloom_cases as bc  # noqa: E402
from tests.helpers import load_tokenizer_json  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def layout():
    d = json.loads(load_tokenizer_json("split_qwen2"))
    nxt = max(d["model"]["vocab"].values()) + 1
    added = [(bc.BOS, True), (bc.EOS, True), (bc.PAD, True), (bc.USER, False), (bc.ASSISTANT, False)]
    d["added_tokens"] = [{"id": nxt + k, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": s}
                         for k, (c, s) in enumerate(added)]
    d["normalizer"] = None
    d["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [
        {"type": "Split", "pattern": {"Regex": bc.PATTERN}, "behavior": "Isolated", "invert": False},
        {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}]}
    d["decoder"] = {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": False}
    d["post_processor"] = {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": False, "use_regex": False}
    return json.dumps(d, ensure_ascii=False), nxt + 2


def flat(e):
    return [x for o in e.offsets for x in o]


def arrays(encs):
    return {"ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs]}


def emit(name):
    js, pad_id = layout()
    tok = Tokenizer.from_str(js)
    v = {"reference": f"tokenizers=={tokenizers.__version__}"}
    dd = bc.short_docs() + synth.gen_lines(40, text_seed=91) + bc.random_strings(60, seed=92, lo=10, hi=90)
    v["docs"] = dd
    v.update(arrays(tok.encode_batch(dd, add_special_tokens=False)))
    v["decoded"] = tok.decode_batch(v["ids"], skip_special_tokens=False)
    v["decoded_skip"] = tok.decode_batch(v["ids"], skip_special_tokens=True)
    v["batches"] = [arrays(tok.encode_batch(b, add_special_tokens=False)) for b in bc.batches()]
    # every edge document alone: at byte 0 of its batch
    v["edge"] = arrays([tok.encode(d, add_special_tokens=False) for d in bc.device_edge_docs()])
    big = bc.big_doc()
    v["big"] = dict(arrays([tok.encode(big, add_special_tokens=False)]), n_bytes=len(big.encode("utf-8")))
    small = [d for d in dd if len(d) < 120]
    pairs = [(small[i], small[(i * 7 + 3) % len(small)]) for i in range(0, len(small), 4)]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = dict(arrays(encs), inputs=[list(p) for p in pairs], type_ids=[e.type_ids for e in encs], sequence_ids=[e.sequence_ids for e in encs])
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
    t4.enable_padding(pad_id=pad_id, pad_token=bc.PAD)
    encs = t4.encode_batch(small, add_special_tokens=True)
    v["pad"] = {"pad_id": pad_id, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs], "offsets_char": [flat(e) for e in encs]}
    t5 = Tokenizer.from_str(js)
    t5.enable_truncation(max_length=12)
    t5.enable_padding(pad_id=pad_id, pad_token=bc.PAD, length=12, direction="left")
    encs = t5.encode_batch(small, add_special_tokens=True)
    v["pad_fixed_left"] = {"length": 12, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs],
                           "special_tokens_mask": [e.special_tokens_mask for e in encs]}
    words_in = [["a  b", "x. y"], ["a", " ", "b c"], ["(|)[]", "  ", "it's fine, ok"], ["plain", "words"], [""], ["a" * 70, " " * 70 + "b"], [bc.USER + "a", "b ."], ["中文。", "、，x"]]
    v["pretok"] = dict(arrays(tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)), inputs=words_in)
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    emit(bc.NAME)
