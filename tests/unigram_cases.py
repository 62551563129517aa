"""Inputs the Unigram fixtures and tests share (tools/make_golden_unigram.py writes the expected results of long_docs() into every
fixture's `long` section; tests/test_unigram_gpu.py builds the same documents again instead of carrying 100 KB of them three times)."""
import random


def long_docs():
    """pre-tokens of exactly 8,192 and 8,193 bytes, and one of about 20 KB with chars the vocabularies lack"""
    rng = random.Random(74)
    blob = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789-中文ꙮé😀") for _ in range(9000))
    while len(blob.encode("utf-8")) > 20000:
        blob = blob[:-1]
    cjk = "".join(rng.choice("中文字符日本語のテキスト这是一个用于测试的句子") for _ in range(3000))
    return ["a" * 8189, "b" * 8190, "x " + "d" * 8189 + " " + "a" * 8190 + " y", blob, cjk, "ab " * 3000,
            "hello " * 3000,                                                   # one word thousands of times: the in-batch claims
            " ".join(rng.choice(["hello", "world", "ab", "ddd", "中文", "naïve"]) for _ in range(2000))]
