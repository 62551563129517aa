#!/usr/bin/env python3
"""Golden fixtures for SentencePiece-style BPE converted to tokenizer.json (Llama-2, Mistral, Gemma-style): BPE over characters with
unk_token <unk>, byte_fallback and fuse_unk, behind the "▁" front of the pipeline in its three layouts:
    spm_bpe_llama2        normalizer Sequence[Prepend("▁"), Replace(" " -> "▁")], pre_tokenizer null  (the legacy conversion)
    spm_bpe_first         normalizer null, Metaspace(prepend_scheme "first", split false)             (legacy=false)
    spm_bpe_split         normalizer null, Metaspace(prepend_scheme "always", split true)
    spm_bpe_replace_only  normalizer Replace(" " -> "▁"), pre_tokenizer null
All four share the Llama decoder and post-processor.  Written with the REFERENCE wheel:
    tests/golden/<name>.json.gz, tests/golden/<name>_vectors.json.gz
(ids, byte + char offsets, word ids, decode output; pairs with the template, truncation with stride / overflowing, padding;
pre-tokenized input); tests/golden/spm_bpe_long_vectors.json.gz: units beyond 8 KB in all four layouts.  Runs only where the wheel
is importable.  (`long`: the long units' vectors alone.)"""
import copy
import gzip
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer, models, pre_tokenizers, trainers  # noqa: E402

from oracle import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["spm_bpe_llama2", "spm_bpe_first", "spm_bpe_split", "spm_bpe_replace_only"]
MS = "▁"

MULTI = ["Das ist ein kleiner Test für die Straße.", "Ça va très bien, merci beaucoup!", "Это простой русский текст для проверки.",
         "这是一个用于测试的中文句子。", "日本語のテキストもあります。", "한국어 문장도 하나 넣습니다.", "Ελληνικά γράμματα εδώ.",
         "emoji 😀 and 🎉 here", "naïve café résumé", "中文字符 and English mixed 中文"]


def train_base():
    t = Tokenizer(models.BPE(unk_token="<unk>", byte_fallback=True, fuse_unk=True))
    t.pre_tokenizer = pre_tokenizers.Metaspace(replacement=MS, prepend_scheme="always", split=True)
    corpus = synth.gen_lines(6000, text_seed=61) + MULTI * 40
    t.train_from_iterator(corpus, trainers.BpeTrainer(vocab_size=3000, special_tokens=["<unk>", "<s>", "</s>"], limit_alphabet=200, show_progress=False))
    d = json.loads(t.to_str())
    vocab = d["model"]["vocab"]
    nxt = max(vocab.values()) + 1
    for b in range(256):
        key = "<0x%02X>" % b
        if key not in vocab:
            vocab[key] = nxt
            nxt += 1
    d["model"]["byte_fallback"] = True
    d["model"]["fuse_unk"] = True
    d["model"]["unk_token"] = "<unk>"
    d["decoder"] = {"type": "Sequence", "decoders": [
        {"type": "Replace", "pattern": {"String": MS}, "content": " "}, {"type": "ByteFallback"}, {"type": "Fuse"},
        {"type": "Strip", "content": " ", "start": 1, "stop": 0}]}
    d["post_processor"] = {
        "type": "TemplateProcessing",
        "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}],
        "pair": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                 {"SpecialToken": {"id": "<s>", "type_id": 1}}, {"Sequence": {"id": "B", "type_id": 1}}],
        "special_tokens": {"<s>": {"id": "<s>", "ids": [vocab["<s>"]], "tokens": ["<s>"]}}}
    return d


def layout(base, name):
    d = copy.deepcopy(base)
    rep = {"type": "Replace", "pattern": {"String": " "}, "content": MS}
    if name == "spm_bpe_llama2":
        d["normalizer"] = {"type": "Sequence", "normalizers": [{"type": "Prepend", "prepend": MS}, rep]}
        d["pre_tokenizer"] = None
    elif name == "spm_bpe_first":
        d["normalizer"] = None
        d["pre_tokenizer"] = {"type": "Metaspace", "replacement": MS, "prepend_scheme": "first", "split": False}
    elif name == "spm_bpe_split":
        d["normalizer"] = None
        d["pre_tokenizer"] = {"type": "Metaspace", "replacement": MS, "prepend_scheme": "always", "split": True}
    else:
        d["normalizer"] = rep
        d["pre_tokenizer"] = None
    return json.dumps(d, ensure_ascii=False)


def docs():
    random.seed(62)
    edge = ["", " ", "  ", "   ", "Hello world", "  two  spaces ", " leading", "trailing ", "a  b", "tab\there", "new\nline", "\t\n", " \t x \n ",
            f"already{MS}has{MS}{MS}bars", f"{MS}", f"{MS} {MS}", f" {MS}x", "a<s>b c", "<s>", "<s><s>", "x</s>", "</s> y", " <s> a </s> ",
            "a <s>b</s> c", "<unk>", "中文字符 x", "中文字符", "日本語のテキスト", "😀", "emoji 😀 here", "🦀🦀 crab", "ࠀࠁ rare",
            "ꙮꙮꙮ ꙮ", "naïve café", "x" * 70, "ab " * 40, "é" * 30]
    base = synth.gen_lines(120, text_seed=63)
    pool = ["a", "b", " ", "  ", "\t", "\n", MS, "<s>", "</s>", "中", "文", "😀", "ꙮ", "é", "the", "ing", "x", "Hello", "world", "ß", "ё"]
    mixed = ["".join(random.choice(pool) for _ in range(random.randint(1, 14))) for _ in range(300)]
    return edge + MULTI + base + mixed


def enc_fields(encs, texts):
    ids, offs, coffs, words = [], [], [], []
    for e, d in zip(encs, texts):
        m = [0]
        for ch in d:
            m.append(m[-1] + len(ch.encode("utf-8")))
        ids.append(e.ids)
        coffs.append([[a, b] for a, b in e.offsets])
        offs.append([[m[a], m[b]] for a, b in e.offsets])
        words.append(e.word_ids)
    return ids, offs, coffs, words


def emit(name, tok_json, dd):
    tok = Tokenizer.from_str(tok_json)
    encs = tok.encode_batch(dd, add_special_tokens=False)
    ids, offs, coffs, words = enc_fields(encs, dd)
    v = {"docs": dd, "ids": ids, "offsets": offs, "offsets_char": coffs, "words": words,
         "decoded": tok.decode_batch(ids, skip_special_tokens=False), "reference": f"tokenizers=={tokenizers.__version__}"}
    # add_special_tokens=True: the template's <s> in front
    encs = tok.encode_batch(dd, add_special_tokens=True)
    v["special"] = {"ids": [e.ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    # pairs with the pair template, then truncation with stride + overflowing, then padding
    pairs = [(dd[i], dd[(i * 7 + 3) % len(dd)]) for i in range(0, min(len(dd), 160))]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = {"inputs": [list(p) for p in pairs], "ids": [e.ids for e in encs], "type_ids": [e.type_ids for e in encs],
                  "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    t2 = Tokenizer.from_str(tok_json)
    t2.enable_truncation(max_length=12, stride=3)
    single = dd[:160]
    encs = t2.encode_batch(single, add_special_tokens=True)
    v["trunc"] = {"max_length": 12, "stride": 3, "ids": [e.ids for e in encs],
                  "overflowing": [[o.ids for o in e.overflowing] for e in encs]}
    t3 = Tokenizer.from_str(tok_json)
    t3.enable_padding(pad_id=0, pad_token="<unk>")
    encs = t3.encode_batch(single, add_special_tokens=True)
    v["pad"] = {"ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs]}
    # pre-tokenized input: every word is its own piece at offset 0
    words_in = [["ab", "cd ef"], ["Hello", "world"], [" x", "y "], ["中文", "<s>", "a"], [""], ["a b c"]]
    encs = tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)
    v["pretok"] = {"inputs": words_in, "ids": [e.ids for e in encs], "words": [e.word_ids for e in encs],
                   "offsets_char": [[list(o) for o in e.offsets] for e in encs]}
    for fn, text in ((name + ".json.gz", tok_json), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
    print(name, "vocab", tok.get_vocab_size(), "docs", len(dd))


def long_docs():
    """Units beyond the LDS kernels' 8 KB: a CJK paragraph (no spaces: one unit), a 20 KB blob without spaces (with chars the vocabulary
    lacks: byte fallback, inside the unit), documents of exactly 8,192 / 8,193 bytes, and units of exactly 8,192 / 8,193 bytes of X."""
    rng = random.Random(64)
    blob = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789-中文ꙮé😀") for _ in range(9000))
    while len(blob.encode("utf-8")) > 20000:
        blob = blob[:-1]
    blob += "z" * (20000 - len(blob.encode("utf-8")))
    cjk = "".join(rng.choice("中文字符日本語のテキスト这是一个用于测试的句子") for _ in range(10000))
    return [cjk, blob, "a" * 8192, "a" * 8193, "a" * 8189, "a" * 8190, "b" * 8188 + " c", "x " + "中" * 3000 + " y <s>" + "文" * 2731 + "</s>", "ab " * 3000]


def emit_long(base):
    dd = long_docs()
    v = {"docs": dd, "reference": f"tokenizers=={tokenizers.__version__}"}
    for name in NAMES:
        # (ids and char offsets in every layout, word ids where they are not all 0; byte offsets follow from the char offsets)
        tok = Tokenizer.from_str(layout(base, name))
        ids, _, coffs, words = enc_fields(tok.encode_batch(dd, add_special_tokens=False), dd)
        v[name] = {"ids": ids, "offsets_char": [[x for o in c for x in o] for c in coffs]}
        if any(any(w) for w in words):
            v[name]["words"] = words
    with gzip.GzipFile(os.path.join(GOLD, "spm_bpe_long_vectors.json.gz"), "wb", mtime=0) as fh:
        fh.write(json.dumps(v, ensure_ascii=False).encode("utf-8"))
    print("spm_bpe_long_vectors", "docs", len(dd))


def main():
    base = train_base()
    if len(sys.argv) > 1 and sys.argv[1] == "long":       # (the long units' vectors alone: the fixtures above stay byte for byte)
        emit_long(base)
        return
    dd = docs()
    for name in NAMES:
        emit(name, layout(base, name), dd)
    emit_long(base)


if __name__ == "__main__":
    main()
