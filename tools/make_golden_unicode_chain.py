#!/usr/bin/env python3
"""Golden fixtures for the NFD / Lowercase / StripAccents normalizer chains, written with the REFERENCE wheel:
    chain_nls_wp    Sequence[NFD, Lowercase, StripAccents], Whitespace, WordPiece, a [CLS] A [SEP] template
    chain_l_wl      Lowercase, WhitespaceSplit, WordLevel
    chain_sl_bpe    Sequence[StripAccents, Lowercase], BertPreTokenizer, BPE over characters with an unk_token, one raw and one
                    normalized added token
    chain_nl_wp     Sequence[NFD, Lowercase] -- NFD stays visible: the NFC normalizer's segments in their NFD mode --, Whitespace, WordPiece,
                    one raw added token; its batch also holds tests/nfc_cases.py straddle_docs() and marks out of canonical order
Each reuses the vocabulary of an existing fixture (at most 4,000 entries) with a few pieces of normalized text put in.
tests/golden/<name>.json.gz, tests/golden/<name>_vectors.json.gz: ids, char offsets (flat pairs; the byte offsets follow from them), word
ids of tests/unicode_chain_cases.py batch_docs(); one case each with the special tokens, pairs, truncation with stride and overflow, and
pre-tokenized input.  Runs only where the wheel is importable."""
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
from tests import unicode_chain_cases as uc  # noqa: E402
from tests.helpers import load_tokenizer_json  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["chain_nls_wp", "chain_l_wl", "chain_sl_bpe", "chain_nl_wp"]


def _added(i, content, normalized, special):
    return {"id": i, "content": content, "single_word": False, "lstrip": False, "rstrip": False, "normalized": normalized, "special": special}


def _replace_tail(vocab, pieces, keep):
    """the vocabulary cut to `keep` entries, then `pieces` on the ids that follow"""
    v = {t: i for t, i in vocab.items() if i < keep}
    for p in pieces:
        if p not in v:
            v[p] = len(v)
    assert sorted(v.values()) == list(range(len(v))) and len(v) <= 4000
    return v


def layout(name):
    if name == "chain_nls_wp":
        d = json.loads(load_tokenizer_json("bert_wordpiece_4000"))
        d["normalizer"] = uc.sequence("NLS")
        d["pre_tokenizer"] = {"type": "Whitespace"}
        d["model"]["vocab"] = _replace_tail(d["model"]["vocab"], ["\u1112", "##\u1161", "##\u11ab", "\u1100", "##\u1165", "\u03b9", "\u03b1", "\u03bf\u03b4\u03bf\u03c3",
                                                                  "\u1112\u1161\u11ab", "cafe", "istanbul", "strasse", "##\u00df", "\u0915"], 3980)
        d["post_processor"] = {
            "type": "TemplateProcessing",
            "single": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}}],
            "pair": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}},
                     {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
            "special_tokens": {c: {"id": c, "ids": [i], "tokens": [c]} for c, i in (("[CLS]", 2), ("[SEP]", 3))}}
        pad = ("[PAD]", 0)
    elif name == "chain_nl_wp":
        d = json.loads(load_tokenizer_json("bert_wordpiece_4000"))
        d["normalizer"] = uc.sequence("NL")
        d["pre_tokenizer"] = {"type": "Whitespace"}
        d["model"]["vocab"] = _replace_tail(d["model"]["vocab"], ["\u0301", "##\u0301", "##\u0316", "\u0316", "##\u0307", "##\u0327", "\u1112", "##\u1161", "##\u11ab", "\u1100",
                                                                  "\u03b9", "##\u0308", "e\u0301", "cafe\u0301", "##\u0345", "##\u030a", "\u0915", "##\u093c"], 3970)
        d["added_tokens"] = list(d["added_tokens"]) + [_added(len(d["model"]["vocab"]), uc.RAW_TOKEN, False, True)]
        pad = ("[PAD]", 0)
    elif name == "chain_l_wl":
        d = json.loads(load_tokenizer_json("wordlevel_wssplit"))
        d["normalizer"] = uc.L
        d["model"]["vocab"] = _replace_tail(d["model"]["vocab"], ["caf\u00e9", "i\u0307stanbul", "i\u0307", "\u00e9", "\u03bf\u03b4\u03bf\u03c3", "\ud55c", "stra\u00dfe", "\u00df",
                                                                  "\u00e1b", "\u0301", "mixedcase", "tail", "start\u00e9"], 3300)
        pad = (d["model"]["unk_token"], d["model"]["vocab"][d["model"]["unk_token"]])
    else:
        d = json.loads(load_tokenizer_json("bpe_ws_unk"))
        d["normalizer"] = uc.sequence("SL")
        d["pre_tokenizer"] = {"type": "BertPreTokenizer"}
        v = d["model"]["vocab"]
        for p in ["\u0307", "\ud55c", "\u03c3", "\u00e1", "\u00df"]:
            v.setdefault(p, len(v))
        n = len(v)
        d["added_tokens"] = list(d["added_tokens"]) + [_added(n, uc.RAW_TOKEN, False, True), _added(n + 1, uc.NORM_TOKEN, True, False)]
        pad = ("[UNK]", v["[UNK]"])
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
    prose = synth.gen_lines(70, text_seed=73)
    prose = [p.replace("e", "\u00e9", 1).title() if k % 3 == 0 else p for k, p in enumerate(prose)]
    dd = uc.batch_docs(prose)
    if name == "chain_nl_wp":
        dd = dd + nfc_cases.straddle_docs() + uc.out_of_order_docs()
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
    words_in = [["\u00c9", "\u0301x"], ["CAF\u00c9", "au", "lait"], ["\u0301", "B"], ["\ud55c\uad6d", "\u0130"], ["plain", "Words"], [""], ["a" + uc.RAW_TOKEN, "Caf\u00e9"]]
    encs = tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)
    v["pretok"] = {"inputs": words_in, "ids": [e.ids for e in encs], "words": [e.word_ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs]}
    for fn, text in ((name + ".json.gz", js), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    for n in NAMES:
        emit(n)
