"""Shared by the tests of the NFKC normalizer in front of the "▁" front (NORM_NFKC: the K mode of csrc/nfc_core.hpp, kernels/nfkc.hip)
and by tools/make_golden_nfkc.py: small tokenizer files around NFKC, the chars NFKC changes -- each put where the kernels can go wrong --,
runs of them that the widened head rule must cut, and seeded strings."""
import json
import random

from tests import nfc_cases
from tests import unicode_chain_cases as uc

K = {"type": "NFKC"}
MS = {"type": "Metaspace", "replacement": "\u2581", "prepend_scheme": "always", "split": True}
CBPE = {"type": "BPE", "vocab": {"<unk>": 0, "\u2581": 1, "a": 2, "c": 3, "f": 4, "i": 5, "e": 6, "ca": 7, "fi": 8, "A": 9}, "merges": [["c", "a"], ["f", "i"]], "unk_token": "<unk>"}
UNI = {"type": "Unigram", "unk_id": 0, "vocab": [["<unk>", 0.0], ["\u2581", -2.0], ["\u2581a", -1.0], ["fi", -1.5], ["a", -3.0], ["f", -3.0], ["i", -3.0]], "byte_fallback": False}
MODELS = {"bpe_chars": CBPE, "unigram": UNI}


def file_of(norm=K, model=CBPE, pre=MS, added=()):
    return json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": list(added), "normalizer": norm, "pre_tokenizer": pre,
                       "post_processor": None, "decoder": None, "model": model}, ensure_ascii=False)


def char_isolating_file():
    """a WordLevel file behind NFKC whose pre-tokenizer isolates every char and whose vocabulary knows none: one <unk> per normalized char,
    its offsets the source range the reference's NormalizedString aligns that char to (the strings hold no newline)"""
    return json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": K,
                       "pre_tokenizer": {"type": "Split", "pattern": {"Regex": "."}, "behavior": "Isolated", "invert": False},
                       "post_processor": None, "decoder": None, "model": {"type": "WordLevel", "vocab": {"<unk>": 0}, "unk_token": "<unk>"}})


FI, FW_A, IDSP, NBSP, SALLA, LONG_S, SQUARE = "\ufb01", "\uff21", "\u3000", "\u00a0", "\ufdfa", "\u1e9b\u0323", "\u3300"
JAMO, E_ACUTE = "\u1100\u1161\u11a8", "e\u0301"
# the chars the issue names: 3 bytes -> 2, 3 -> 1, two that become a space (the front must split there), 3 -> 33, one that reorders and
# composes, one char -> several, Hangul jamo L V T, a base and a mark that compose
OUT_OF_ORDER = ["e\u0301\u0316", "a\u0345\u0301\u0316"]          # marks out of canonical order (unicode_chain_cases.out_of_order_docs)
CHANGING = [FI, FW_A, IDSP, NBSP, SALLA, LONG_S, SQUARE, JAMO, E_ACUTE] + OUT_OF_ORDER
RAW_TOKEN, NORM_TOKEN = "<raw>", "\uff23af\u00e9"          # the normalized token's pattern is "Caf\u00e9"

BASES = uc.BASES + [FI, FW_A, IDSP, NBSP, SALLA, "\u1e9b", SQUARE, "\u1100", "\u3131", "\uff76", "\u2460", "\u00bd", "\u2126", "\ufb03", "\u0132", "\uff9e", "\u00b5", " "]
MARKS = uc.MARKS + ["\u1161", "\u11a8", "\uff9f", "\u0323", "\u3099", "\u309b"]


def seeded_strings(n, seed):
    """bases -- among them the chars NFKC changes on their own -- and marks, jamo and halfwidth voicing marks, in and out of order"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = []
        for _ in range(rng.randint(1, 8)):
            if rng.random() < 0.8:
                s.append(rng.choice(BASES))
            for _ in range(rng.choice((0, 0, 1, 2, 3))):
                s.append(rng.choice(MARKS))
        out.append("".join(s))
    return out


def straddle_docs():
    """every changing char ENDING at and STRADDLING (beginning one byte before) a 16-byte lane, a 64-byte mask word and a 4,096-byte
    workgroup boundary of the text -- the document first in its batch --, first and last in a document, alone; and the NFC tests' two
    segments at the same places"""
    out = uc.straddle_docs(CHANGING, [])
    for c in CHANGING:
        n = len(c.encode("utf-8"))
        out.append(uc._filled(4096 - n) + c + "z tail")
        out.append(uc._filled(4095) + c + " tail")
    return out + nfc_cases.straddle_docs()


FULLWIDTH_200 = "".join(chr(0xFF21 + k % 26) for k in range(200))
MIXED_300 = "".join((chr(0xFF41 + k % 26), FI, "\ufb03", chr(0xFF10 + k % 10), "\u2460")[k % 5] for k in range(300))
FIVE_SALLA = "ab" + SALLA * 5 + " x"                       # five U+FDFA in one 16-byte lane and the one behind it: 15 bytes -> 165


def long_run_docs():
    """runs of chars that change on their own, without a space: the widened head rule cuts them char by char (neither may be refused)"""
    return [FULLWIDTH_200, MIXED_300, "x" + FULLWIDTH_200 + " y " + MIXED_300, FIVE_SALLA, SALLA * 5]


ONLY_MARKS = ["\u0301", "\u0316\u0301", "\u3099\u0301", "\uff9e\uff9f"]


# documents that are only marks or empty, and the chars that become a space -- the front must split there and prepend its U+2581, the
# word's offsets on the source char -- at every place of a word
SPACE_DOCS = ["", ""] + ONLY_MARKS + ["a \u0316\u0301 b", "\u0301 x", "x \u0301", IDSP, NBSP + NBSP, "a" + IDSP + "b", "a" + NBSP + "b" + IDSP,
                                      IDSP + "start", "end" + NBSP, "a" + IDSP + IDSP + "b", " " + IDSP + " x"]
# a mark behind a raw added-token match and at a document's start; chars that change around a raw match
RAW_DOCS = [RAW_TOKEN + "\u0301 x", "a" + RAW_TOKEN + "\u0301", "\u0301" + RAW_TOKEN, "\u00c9" + RAW_TOKEN + "\u0316\u0301e", FW_A + RAW_TOKEN + FI, RAW_TOKEN + IDSP + RAW_TOKEN]
# the normalized added token in several spellings: composed, fullwidth + decomposed, fullwidth throughout (twice in one document), inside a word
NORM_DOCS = ["Caf\u00e9 au lait", "a \uff23afe\u0301 b", "Cafe\u0301 \uff23\uff41\uff46\u00e9", "xCaf\u00e9x", "\uff23af\u00e9" + RAW_TOKEN]


def edge_docs():
    """what every fixture encodes: the straddling documents, the long runs, empty documents and documents that are only marks, the chars
    that become a space at every place of a word, marks behind a raw added-token match and at a document's start, the normalized added
    token in several spellings, and compatibility chars of every kind"""
    d = straddle_docs() + long_run_docs() + SPACE_DOCS + RAW_DOCS + NORM_DOCS
    d += ["\uff28\uff45\uff4c\uff4c\uff4f\u3000\uff37\uff4f\uff52\uff4c\uff44\uff01", "\uff8a\uff9f\uff70\uff84 \uff76\uff9e", "\u3131\u314f \u1100\u1161 \u1100\u1161\u11a8 \ud55c\uad6d\uc5b4",
          "\u2460\u2461 \u00bd \u2126 \u00b5 \u2122 \u2025", "\u0132sselmeer e\ufb03cient \ufb01\ufb02", "x\u00b2 + y\u00b3 H\u2082O", "\u1e9b\u0323 \u1e9b \u017f\u0323\u0307",
          "\u3300 \u3392 \u33a1", SALLA + " x " + SALLA, "tabs\tand\nnewlines\r\n", "\u4e2d\u6587 \U0001f600 ok", "\U0001d400\U0001d401 \U0001d7ce"]
    d += uc.out_of_order_docs() + ["A" + uc.MARKS30 + " b", FW_A + uc.MARKS30 + IDSP + "b"]
    return d


def batch_docs(prose):
    """the fixtures' batch: more than two workgroups of text (4,096 bytes each), a document count that is no multiple of 256"""
    d = edge_docs() + list(prose)
    while len(d) % 256 in (0, 255):
        d.append("pad" + FI)
    return d
