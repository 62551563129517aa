#!/usr/bin/env python3
"""Golden fixtures for the CLIP layout, written with the REFERENCE wheel:
    clip_bpe         Sequence[NFC, Replace(Regex "\\s+" -> " "), Lowercase] + Sequence[Split(the CLIP pattern, Removed, inverted),
                     ByteLevel(add_prefix_space=false, use_regex=true)] + byte-level BPE with end_of_word_suffix "</w>", RobertaProcessing
                     (trim_offsets false), a ByteLevel decoder, and CLIP's two added tokens: "<|startoftext|>" normalized = true,
                     "<|endoftext|>" normalized = false
    clip_bpe_plain   the same with "<|startoftext|>" normalized = false (decode_batch is on the path there)
over the synthetic vocabulary of tests/clip_cases.py (256 byte chars, their 256 "</w>" forms, greedy merges over a word list).
tests/golden/<name>.json.gz and <name>_vectors.json.gz: ids, char offsets (flat pairs; the byte offsets follow from them and the text) and
word ids of tests/clip_cases.py all_docs(); the same with the special tokens (type ids, special-tokens masks) and as pairs through the
Roberta template for the short ones; prompts with truncation to 77 and padding to 77, as CLIP batches run; decode_batch of the plain
variant.  Reads nothing but the wheel and tests/clip_cases.py; runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from tests import clip_cases as cc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def flat(e):
    return [x for o in e.offsets for x in o]


def arrays(encs):
    return {"ids": [e.ids for e in encs], "offsets_char": [flat(e) for e in encs], "words": [e.word_ids for e in encs]}


def emit(name, normalized_sot):
    js = cc.file_of(normalized_sot=normalized_sot)
    tok = Tokenizer.from_str(js)
    eot = tok.token_to_id(cc.EOT)
    docs = cc.all_docs() if normalized_sot else [d for d in cc.all_docs() if len(d) < 400]
    v = {"reference": f"tokenizers=={tokenizers.__version__}", "docs": docs}
    v.update(arrays(tok.encode_batch(docs, add_special_tokens=False)))
    small = [d for d in docs if len(d) < 160]
    encs = tok.encode_batch(small, add_special_tokens=True)
    v["special"] = dict(arrays(encs), docs=small, type_ids=[e.type_ids for e in encs], special_tokens_mask=[e.special_tokens_mask for e in encs])
    pairs = [(small[i], small[(i * 7 + 3) % len(small)]) for i in range(0, len(small), 3)]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = dict(arrays(encs), inputs=[list(p) for p in pairs], type_ids=[e.type_ids for e in encs], special_tokens_mask=[e.special_tokens_mask for e in encs],
                      sequence_ids=[e.sequence_ids for e in encs])
    t2 = Tokenizer.from_str(js)
    t2.enable_truncation(max_length=77)
    t2.enable_padding(pad_id=eot, pad_token=cc.EOT, length=77)
    prompts = cc.prompts() + small[:40]
    encs = t2.encode_batch(prompts, add_special_tokens=True)
    v["clip77"] = dict(arrays(encs), docs=prompts, max_length=77, pad_id=eot, pad_token=cc.EOT, attention_mask=[e.attention_mask for e in encs],
                       special_tokens_mask=[e.special_tokens_mask for e in encs])
    if not normalized_sot:
        keep = [i for i, d in enumerate(docs) if len(d) < 400]
        v["decode"] = {"index": keep, "decoded": tok.decode_batch([v["ids"][i] for i in keep], skip_special_tokens=False),
                       "decoded_skip": tok.decode_batch([v["ids"][i] for i in keep], skip_special_tokens=True)}
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    emit("clip_bpe", True)
    emit("clip_bpe_plain", False)
