#!/usr/bin/env python3
"""Golden fixtures for the NFC normalizer in front of byte-level BPE, written with the REFERENCE wheel:
    nfc_qwen2   the Qwen2 layout: NFC, Sequence[Split(Qwen2 pattern), ByteLevel(use_regex=false)], normalized=false specials, a template
    nfc_gpt2    NFC, ByteLevel (GPT-2 regex) with trim_offsets, a ByteLevel post-processor, and one normalized=true added token
Both reuse the vocabulary of tests/golden/split_qwen2.json.gz.  tests/golden/<name>.json.gz, tests/golden/<name>_vectors.json.gz:
ids, char offsets (flat pairs; the byte offsets follow from them), word ids of tests/nfc_cases.py edge_docs() and some prose; one case each with the special tokens, pairs,
truncation + padding, and pre-tokenized input.  Runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from oracle import synth  # noqa: E402
from tests import nfc_cases  # noqa: E402
from tests.helpers import load_tokenizer_json  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["nfc_qwen2", "nfc_gpt2"]


def layout(name):
    d = json.loads(load_tokenizer_json("split_qwen2"))
    nxt = max(d["model"]["vocab"].values()) + 1
    sp = ["<|endoftext|>", "<|im_start|>", "<|im_end|>"]
    d["added_tokens"] = [{"id": nxt + k, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}
                         for k, c in enumerate(sp)]
    d["normalizer"] = {"type": "NFC"}
    if name == "nfc_qwen2":
        d["post_processor"] = {
            "type": "TemplateProcessing",
            "single": [{"SpecialToken": {"id": "<|im_start|>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "<|im_end|>", "type_id": 0}}],
            "pair": [{"SpecialToken": {"id": "<|im_start|>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "<|im_end|>", "type_id": 0}},
                     {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "<|im_end|>", "type_id": 1}}],
            "special_tokens": {c: {"id": c, "ids": [nxt + k], "tokens": [c]} for k, c in enumerate(sp) if k}}
    else:
        d["normalizer"] = {"type": "Sequence", "normalizers": [{"type": "NFC"}]}
        d["pre_tokenizer"] = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}
        d["post_processor"] = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}
        d["added_tokens"].append({"id": nxt + 3, "content": "caf\u00e9 au", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False})
        d["added_tokens"].append({"id": nxt + 4, "content": "e\u0301e", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False})
    return json.dumps(d, ensure_ascii=False), nxt


def fields(encs, texts):
    out = {"ids": [], "offsets_char": [], "words": []}      # (byte offsets follow from the char offsets and the text: tests.helpers.char_to_byte)
    for e, t in zip(encs, texts):
        out["ids"].append(e.ids)
        out["offsets_char"].append([x for o in e.offsets for x in o])
        out["words"].append(e.word_ids)
    return out


def emit(name):
    js, pad_id = layout(name)
    tok = Tokenizer.from_str(js)
    dd = nfc_cases.edge_docs() + synth.gen_lines(40, text_seed=71) + nfc_cases.random_segments(60, seed=72)
    v = {"docs": dd, "reference": f"tokenizers=={tokenizers.__version__}"}
    v.update(fields(tok.encode_batch(dd, add_special_tokens=False), dd))
    small = [d for d in dd if len(d) < 200]
    encs = tok.encode_batch(small, add_special_tokens=True)
    v["special"] = {"docs": small, "ids": [e.ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    pairs = [(small[i], small[(i * 7 + 3) % len(small)]) for i in range(0, len(small), 2)]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = {"inputs": [list(p) for p in pairs], "ids": [e.ids for e in encs], "type_ids": [e.type_ids for e in encs],
                  "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    t2 = Tokenizer.from_str(js)
    t2.enable_truncation(max_length=9, stride=2)
    t2.enable_padding(pad_id=pad_id, pad_token="<|endoftext|>")
    encs = t2.encode_batch(small, add_special_tokens=True)
    v["trunc_pad"] = {"max_length": 9, "stride": 2, "pad_id": pad_id, "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs],
                      "offsets_char": [[list(o) for o in e.offsets] for e in encs]}
    words_in = [["e\u0301", "\u0301x"], ["cafe\u0301", "au", "lait"], ["\u1100\u1161", "\u11a8"], ["plain", "words"], [""], ["x\u0958y", "\u212b"]]
    encs = tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)
    v["pretok"] = {"inputs": words_in, "ids": [e.ids for e in encs], "words": [e.word_ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs]}
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    for n in NAMES:
        emit(n)
