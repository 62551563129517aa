#!/usr/bin/env python3
"""Golden fixtures for Unigram models (SentencePiece Viterbi) behind Metaspace(split = true), written with the REFERENCE wheel:
    unigram_ms          the piece strings of the committed spm_bpe_llama2 fixture (the 256 <0xXX> pieces among them) with seeded negative
                        scores of 15-17 significant digits, byte_fallback true, the Llama decoder and template
    unigram_ms_nobytes  the same without the <0xXX> pieces: unk runs stay unk
    unigram_adv         a small hand-made vocabulary: exact ties, pieces of 17 / 33 / 70 bytes, multi-byte pieces, every score >= 100 (two unks
                        outscore the pair's own piece, so a fused run is itself a piece), a duplicated piece, the unk piece not at id 0,
                        prepend_scheme "first"
-> tests/golden/<name>.json.gz, tests/golden/<name>_vectors.json.gz (ids, byte + char offsets, word ids, decode output; the template, pairs,
truncation with stride / overflowing, padding; pre-tokenized input; `long`: pre-tokens of 8,192 / 8,193 bytes and about 20 KB, one word
thousands of times).  The vocabularies are synthetic and deterministic: no trainer.  Runs only where the wheel is importable."""
import gzip
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tokenizers  # noqa: E402
from tokenizers import Tokenizer  # noqa: E402

from oracle import synth  # noqa: E402
from tests.unigram_cases import long_docs  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["unigram_ms", "unigram_ms_nobytes", "unigram_adv"]
MS = "▁"
BYTES = ["<0x%02X>" % b for b in range(256)]
MULTI = ["Das ist ein kleiner Test für die Straße.", "Ça va très bien, merci beaucoup!", "Это простой русский текст для проверки.",
         "这是一个用于测试的中文句子。", "日本語のテキストもあります。", "emoji 😀 and 🎉 here", "naïve café résumé", "中文字符 and English mixed 中文"]


def _gz(name):
    with gzip.open(os.path.join(GOLD, name), "rt", encoding="utf-8") as fh:
        return fh.read()


def ms_file(with_bytes: bool) -> str:
    src = json.loads(_gz("spm_bpe_llama2.json.gz"))
    pieces = [p for p, _ in sorted(src["model"]["vocab"].items(), key=lambda kv: kv[1])]
    if not with_bytes:
        pieces = [p for p in pieces if p not in BYTES]
    assert MS in pieces and pieces[0] == "<unk>"
    rng = random.Random(71)
    vocab = []
    for p in pieces:
        # a longer piece costs less per char than the chars it is made of, so natural text comes out in few tokens; 15-17 significant digits
        score = -(2.0 + rng.random() * 6.0 + 0.35 * len(p))
        vocab.append([p, 0.0 if p == "<unk>" else score])
    ids = {p: i for i, (p, _) in enumerate(vocab)}
    d = {"version": "1.0", "truncation": None, "padding": None,
         "added_tokens": [{"id": ids[c], "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}
                          for c in ("<unk>", "<s>", "</s>")],
         "normalizer": None,
         "pre_tokenizer": {"type": "Metaspace", "replacement": MS, "prepend_scheme": "always", "split": True},
         "post_processor": {
             "type": "TemplateProcessing",
             "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}],
             "pair": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                      {"SpecialToken": {"id": "<s>", "type_id": 1}}, {"Sequence": {"id": "B", "type_id": 1}}],
             "special_tokens": {"<s>": {"id": "<s>", "ids": [ids["<s>"]], "tokens": ["<s>"]}}},
         "decoder": {"type": "Sequence", "decoders": [
             {"type": "Replace", "pattern": {"String": MS}, "content": " "}, {"type": "ByteFallback"}, {"type": "Fuse"},
             {"type": "Strip", "content": " ", "start": 1, "stop": 0}]},
         "model": {"type": "Unigram", "unk_id": 0, "vocab": vocab, "byte_fallback": True}}
    return json.dumps(d, ensure_ascii=False)


def adv_file() -> str:
    p17, p33, p70 = "q" * 17, MS + "w" * 30, "z" * 70
    vocab = [[MS, 100.0], ["a", 100.0], ["b", 100.0], ["ab", 200.0],          # an exact tie: a + b against ab
             ["<unk>", 100.0],                                                # the unk piece, not at id 0 (and part of min_score)
             [MS + "a", 200.0], ["c", 100.5], ["abc", 300.5], ["bc", 200.5],  # ties of three ways
             ["xy", 100.0],                                                   # x and y are no pieces: two unks (90 + 90) outscore it, and the fused run IS it
             ["é", 101.0], ["中", 102.0], ["中文", 203.0], ["éa", 201.0], ["😀", 100.25],
             [p17, 1700.0], [p33, 3300.0], [p70, 7000.0], ["q", 100.0], ["w", 100.0], ["z", 100.0],
             ["e", 100.0], ["ee", 200.0], ["e", 150.0],                       # a duplicate: the later id encodes, with ITS score (e + e = 300 beats ee)
             ["d", 100.0], ["dd", 200.0], ["ddd", 300.0],
             ["hello", 500.0], ["h", 100.0], ["l", 100.0], ["o", 100.0]]
    n = len(vocab)
    d = {"version": "1.0", "truncation": None, "padding": None,
         "added_tokens": [{"id": n, "content": "<s>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True},
                          {"id": n + 1, "content": "<x>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False}],
         "normalizer": None,
         "pre_tokenizer": {"type": "Metaspace", "replacement": MS, "prepend_scheme": "first", "split": True},
         "post_processor": {
             "type": "TemplateProcessing",
             "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}],
             "pair": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                      {"SpecialToken": {"id": "<s>", "type_id": 1}}, {"Sequence": {"id": "B", "type_id": 1}}],
             "special_tokens": {"<s>": {"id": "<s>", "ids": [n], "tokens": ["<s>"]}}},
         "decoder": None,
         "model": {"type": "Unigram", "unk_id": 4, "vocab": vocab, "byte_fallback": False}}
    return json.dumps(d, ensure_ascii=False)


def sized_words():
    """words whose pre-token (the "▁" in front included) is exactly 1, 15, 16, 17, 32, 33, 64 and 65 bytes, plain and with chars of 2-4 bytes"""
    out = [MS]
    for n in (15, 16, 17, 32, 33, 64, 65):
        out.append("a" + "b" * (n - 4))                                       # behind a space: "▁" + n - 3 bytes
        out.append("t " + "d" * (n - 3))
        out.append("x " + "é" * ((n - 3) // 2) + "a" * ((n - 3) % 2))
        out.append("x " + "中" * ((n - 3) // 3) + "b" * ((n - 3) % 3))
        out.append("q" * (n - 3) + " " + "z" * (n - 3) + " " + "w" * (n - 3))
    return out


def docs():
    rng = random.Random(72)
    edge = ["", " ", "  ", "   ", "Hello world", "  two  spaces ", " leading", "trailing ", "a  b", "tab\there", "new\nline", "\t\n", " \t x \n ",
            f"already{MS}has{MS}{MS}bars", f"{MS}", f"{MS} {MS}", f" {MS}x", "a<s>b c", "<s>", "<s><s>", "x</s>", "</s> y", " <s> a </s> ", "a <s>b</s> c",
            "<unk>", "qq<unk>", "xx<unk>", "xx<unk>ab", "<unk>qq x<unk>y", "a<x>b hello<x>", "hello hellohello", "e", "ee eee", "ab", "abc", "abcabc ab", "xy", "xyxy axyb", "aa a", "éa éaé",
            "中文字符 x", "中文字符", "中é", "a中éb", "日本語のテキスト", "😀", "emoji 😀 here", "🦀🦀 crab", "ࠀࠁ rare", "ꙮꙮꙮ ꙮ", "naïve café",
            # unk runs at the start, in the middle and at the end of a word, over multi-byte chars and over the 16- / 32-byte marks
            "ꙮabc", "abꙮꙮcd", "abcꙮ", "ꙮ", "ꙮꙮ", "a" * 11 + "ꙮꙮ" + "b" * 5, "d" * 26 + "😀ꙮ" + "d", "b" * 13 + "ꙮ", "ꙮ" + "a" * 28 + "ꙮ", "a" * 60 + "ꙮ🦀ꙮ" + "b" * 9,
            "dddd ddddd dddddd ddddddddd", "x" * 70, "ab " * 40, "é" * 30,
            "hello " * 40]
    base = synth.gen_lines(60, text_seed=73)
    pool = ["a", "b", "c", "d", "ab", "xy", "x", "y", " ", "  ", "\t", "\n", MS, "<s>", "</s>", "<unk>", "<x>", "中", "文", "😀", "ꙮ", "é", "the", "ing", "Hello", "world", "ß", "ё",
            "q" * 17, "w" * 30, "z" * 70, "hello"]
    mixed = ["".join(rng.choice(pool) for _ in range(rng.randint(1, 14))) for _ in range(200)]
    return edge + sized_words() + MULTI + base + mixed


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
    v = {"docs": dd, "ids": ids, "offsets_char": coffs, "words": words,      # (byte offsets follow from the char offsets: the tests convert)
         "decoded": tok.decode_batch(ids, skip_special_tokens=False), "reference": f"tokenizers=={tokenizers.__version__}"}
    encs = tok.encode_batch(dd, add_special_tokens=True)
    v["special"] = {"ids": [e.ids for e in encs], "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    short = [d for d in dd if len(d) < 400]
    pairs = [(short[i], short[(i * 7 + 3) % len(short)]) for i in range(0, min(len(short), 120))]
    encs = tok.encode_batch(pairs, add_special_tokens=True)
    v["pairs"] = {"inputs": [list(p) for p in pairs], "ids": [e.ids for e in encs], "type_ids": [e.type_ids for e in encs],
                  "offsets_char": [[list(o) for o in e.offsets] for e in encs], "words": [e.word_ids for e in encs]}
    t2 = Tokenizer.from_str(tok_json)
    t2.enable_truncation(max_length=12, stride=3)
    single = short[:120]
    encs = t2.encode_batch(single, add_special_tokens=True)
    v["trunc"] = {"inputs": single, "max_length": 12, "stride": 3, "ids": [e.ids for e in encs], "overflowing": [[o.ids for o in e.overflowing] for e in encs]}
    t3 = Tokenizer.from_str(tok_json)
    t3.enable_padding(pad_id=0, pad_token=tok.id_to_token(0))
    encs = t3.encode_batch(single, add_special_tokens=True)
    v["pad"] = {"pad_token": tok.id_to_token(0), "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs]}
    words_in = [["ab", "cd ef"], ["Hello", "world"], [" x", "y "], ["中文", "<s>", "a"], [""], ["a b c"], ["ꙮ", "中é", "xy"]]
    encs = tok.encode_batch(words_in, is_pretokenized=True, add_special_tokens=False)
    v["pretok"] = {"inputs": words_in, "ids": [e.ids for e in encs], "words": [e.word_ids for e in encs],
                   "offsets_char": [[list(o) for o in e.offsets] for e in encs]}
    ld = long_docs()
    lids, _, lcoffs, lwords = enc_fields(tok.encode_batch(ld, add_special_tokens=False), ld)
    v["long"] = {"ids": lids, "offsets_char": [[x for o in c for x in o] for c in lcoffs], "words": lwords}
    for fn, text in ((name + ".json.gz", tok_json), (name + "_vectors.json.gz", json.dumps(v, ensure_ascii=False, separators=(",", ":")))):
        with gzip.GzipFile(os.path.join(GOLD, fn), "wb", mtime=0) as fh:
            fh.write(text.encode("utf-8"))
    print(name, "vocab", tok.get_vocab_size(), "docs", len(dd), "tokens", sum(len(x) for x in ids))


def main():
    dd = docs()
    emit("unigram_ms", ms_file(True), dd)
    emit("unigram_ms_nobytes", ms_file(False), dd)
    emit("unigram_adv", adv_file(), dd)


if __name__ == "__main__":
    main()
