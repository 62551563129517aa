#!/usr/bin/env python3
"""Golden fixtures for the NFKC normalizer in front of bare Metaspace, written with the REFERENCE wheel:
    nfkc_spm_bpe    what the reference's own SentencePieceBPETokenizer class builds -- NFKC, Metaspace(always), BPE over characters with an
                    unk_token -- over the vocabulary and merges of the spm_bpe_llama2 fixture, with one raw and one normalized added token
                    and a <s> $A </s> template
    nfkc_unigram    Sequence[NFKC], Metaspace(first), Unigram with byte_fallback over the unigram_ms vocabulary, one raw added token
tests/golden/<name>.json.gz, tests/golden/<name>_vectors.json.gz: ids, char offsets (flat pairs; the byte offsets follow from them), word
ids of tests/nfkc_cases.py batch_docs(); one case each with the special tokens, pairs, truncation with stride and overflow, and
pre-tokenized input (the layout of tools/make_golden_unicode_chain.py).  Runs only where the wheel is importable."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import SentencePieceBPETokenizer, Tokenizer  # noqa: E402

from oracle import synth  # noqa: E402
from tests import nfkc_cases as kc  # noqa: E402
from tests.helpers import load_tokenizer_json  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["nfkc_spm_bpe", "nfkc_unigram"]
LIMIT = os.path.getsize(os.path.join(GOLD, "spm_bpe_llama2_vectors.json.gz"))


def _added(i, content, normalized, special):
    return {"id": i, "content": content, "single_word": False, "lstrip": False, "rstrip": False, "normalized": normalized, "special": special}


def layout(name):
    if name == "nfkc_spm_bpe":
        base = json.loads(load_tokenizer_json("spm_bpe_llama2"))
        vocab = base["model"]["vocab"]
        merges = [tuple(m) if isinstance(m, list) else tuple(m.split(" ")) for m in base["model"]["merges"]]
        t = SentencePieceBPETokenizer(vocab=vocab, merges=merges, unk_token="<unk>", fuse_unk=True)
        d = json.loads(t.to_str())
        assert d["normalizer"] == {"type": "NFKC"} and d["pre_tokenizer"]["type"] == "Metaspace" and d["model"]["type"] == "BPE"
        n = len(vocab)
        d["added_tokens"] = [a for a in base["added_tokens"]] + [_added(n, kc.RAW_TOKEN, False, True), _added(n + 1, kc.NORM_TOKEN, True, False)]
        sid, eid = vocab["<s>"], vocab["</s>"]
        d["post_processor"] = {
            "type": "TemplateProcessing",
            "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}}],
            "pair": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}},
                     {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "</s>", "type_id": 1}}],
            "special_tokens": {c: {"id": c, "ids": [i], "tokens": [c]} for c, i in (("<s>", sid), ("</s>", eid))}}
        pad = ("<unk>", vocab["<unk>"])
    else:
        d = json.loads(load_tokenizer_json("unigram_ms"))
        d["normalizer"] = {"type": "Sequence", "normalizers": [kc.K]}
        d["pre_tokenizer"] = dict(kc.MS, prepend_scheme="first")
        assert d["model"]["byte_fallback"]
        d["added_tokens"] = list(d["added_tokens"]) + [_added(len(d["model"]["vocab"]), kc.RAW_TOKEN, False, True)]
        pad = ("<unk>", 0)
    return json.dumps(d, ensure_ascii=False), pad


def fields(encs):
    out = {"ids": [], "offsets_char": [], "words": []}      # (byte offsets follow from the char offsets and the text: tests.helpers.char_to_byte)
    for e in encs:
        out["ids"].append(e.ids)
        out["offsets_char"].append([x for o in e.offsets for x in o])
        out["words"].append(e.word_ids)
    return out


def emit(name):
    js, (pad_token, pad_id) = layout(name)
    tok = Tokenizer.from_str(js)
    prose = synth.gen_lines(40, text_seed=79)
    prose = [p.replace("fi", kc.FI).replace(" ", kc.IDSP, 1) if k % 3 == 0 else p for k, p in enumerate(prose)]
    dd = kc.batch_docs(prose)
    assert len(dd) % 256 not in (0, 255) and sum(len(x.encode("utf-8")) for x in dd) > 3 * 4096
    v = {"docs": dd, "reference": f"tokenizers=={tokenizers.__version__}"}
    v.update(fields(tok.encode_batch(dd, add_special_tokens=False)))
    small = [x for x in dd if len(x) < 200]
    encs = tok.encode_batch(small, add_special_tokens=True)
    v["special"] = {"docs": small, "ids": [e.ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs],
                    "tokens": [e.tokens for e in encs]}
    pairs = [(small[i], small[(i * 7 + 3) % len(small)]) for i in range(0, len(small), 2)]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = {"inputs": [list(p) for p in pairs], "ids": [e.ids for e in encs], "type_ids": [e.type_ids for e in encs],
                  "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    t2 = Tokenizer.from_str(js)
    t2.enable_truncation(max_length=9, stride=2)
    t2.enable_padding(pad_id=pad_id, pad_token=pad_token)
    encs = t2.encode_batch(small, add_special_tokens=True)
    v["trunc_pad"] = {"max_length": 9, "stride": 2, "pad_id": pad_id, "pad_token": pad_token, "ids": [e.ids for e in encs],
                      "attention_mask": [e.attention_mask for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs],
                      "overflowing_ids": [[o.ids for o in e.overflowing] for e in encs]}
    words_in = [[kc.FI, "\u0301x"], ["\uff23af\u00e9", "au", "lait"], ["\u0301", "B"], ["\uac00", kc.SALLA], ["plain", "Words"], [""], ["a" + kc.RAW_TOKEN, kc.NORM_TOKEN],
                ["a" + kc.IDSP + "b", kc.NBSP], [kc.FULLWIDTH_200[:40], kc.FW_A + "\u0301"]]
    encs = tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)
    v["pretok"] = {"inputs": words_in, "ids": [e.ids for e in encs], "words": [e.word_ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs]}
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False, separators=(",", ":")))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        size = os.path.getsize(os.path.join(GOLD, fn))
        print(fn, size)
        assert size <= LIMIT, (fn, size, LIMIT)


if __name__ == "__main__":
    for n in NAMES:
        emit(n)
