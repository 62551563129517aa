#!/usr/bin/env python3
"""Golden fixtures for Unigram behind the Precompiled normalizer, written with the REFERENCE wheel from tests/precompiled_cases.py:
    precompiled_xlmr  the layout of xlm-roberta-base: Sequence[Precompiled, Replace(Regex " {2,}")] + Sequence[WhitespaceSplit, Metaspace],
                      the nmt_nfkc-like charsmap, byte_fallback, specials, a template
    precompiled_ms    Precompiled alone in front of bare Metaspace, the adversarial charsmap, an lstrip + rstrip special
-> tests/golden/<name>.json.gz, tests/golden/<name>_vectors.json.gz: ids, char offsets and word ids of the corpus (the token offsets flat,
two numbers a token), with the template, pairs, truncation with stride / overflowing, padding.  Byte offsets follow from the char offsets:
the tests convert.  Runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from tests import precompiled_cases as pc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def fields(encs):
    return {"ids": [e.ids for e in encs], "offsets_char": [[x for o in e.offsets for x in o] for e in encs], "words": [e.word_ids for e in encs]}


def emit(name):
    js = pc.tokenizer_json(name)
    tok = Tokenizer.from_str(js)
    docs = pc.corpus()
    v = {"docs": docs, "reference": f"tokenizers=={tokenizers.__version__}", **fields(tok.encode_batch(docs, add_special_tokens=False))}
    v["special"] = fields(tok.encode_batch(docs, add_special_tokens=True))
    pairs = pc.pairs()
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = {"inputs": [list(p) for p in pairs], "type_ids": [e.type_ids for e in encs], **fields(encs)}
    single = [d for d in docs if len(d) < 400][:160]
    t2 = Tokenizer.from_str(js)
    t2.enable_truncation(max_length=12, stride=3)
    encs = t2.encode_batch(single, add_special_tokens=True)
    v["trunc"] = {"inputs": single, "max_length": 12, "stride": 3, "ids": [e.ids for e in encs], "overflowing": [[o.ids for o in e.overflowing] for e in encs]}
    t3 = Tokenizer.from_str(js)
    t3.enable_padding(pad_id=0, pad_token="<unk>")
    encs = t3.encode_batch(single, add_special_tokens=True)
    v["pad"] = {"pad_token": "<unk>", "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs]}
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False, separators=(",", ":")))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)), "bytes")
    print(name, "docs", len(docs), "tokens", sum(len(x) for x in v["ids"]))


if __name__ == "__main__":
    for n in pc.NAMES:
        emit(n)
