"""Shared by the tests of the NFD / Lowercase / StripAccents normalizer chains (NORM_CHAIN) and by tools/make_golden_unicode_chain.py:
the chains, small tokenizer files around them, the documents that put a char which changes length where the kernels can go wrong, and
seeded strings of bases and marks."""
import json
import random

N, L, S = {"type": "NFD"}, {"type": "Lowercase"}, {"type": "StripAccents"}
MEMBER = {"N": N, "L": L, "S": S}
# context free per source char: no NFD, or StripAccents behind it
CONTEXT_FREE = ["L", "S", "LS", "SL", "NS", "NLS", "NSL", "LNS"]
# NFD with no StripAccents behind it leaves the canonical ordering of marks in the text: the NFC normalizer's segments, not composed
NFD_VISIBLE = ["N", "NL", "LN"]
ACCEPTED = CONTEXT_FREE + NFD_VISIBLE
BARE = ["N", "L", "S"]

WL = {"type": "WordLevel", "vocab": {"<unk>": 0, "a": 1, "cafe": 2, "e": 3}, "unk_token": "<unk>"}
WP = {"type": "WordPiece", "vocab": {"[UNK]": 0, "a": 1, "caf": 2, "##e": 3}, "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100}
CBPE = {"type": "BPE", "vocab": {"<unk>": 0, "a": 1, "c": 2, "f": 3, "e": 4, "ca": 5}, "merges": [["c", "a"]], "unk_token": "<unk>"}
MODELS = {"wordlevel": WL, "wordpiece": WP, "bpe_chars": CBPE}
PRES = [{"type": "Whitespace"}, {"type": "WhitespaceSplit"}, {"type": "BertPreTokenizer"}]


def sequence(chain):
    return {"type": "Sequence", "normalizers": [MEMBER[c] for c in chain]}


def file_of(norm, model=WL, pre=PRES[0], added=()):
    return json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": list(added), "normalizer": norm, "pre_tokenizer": pre,
                       "post_processor": None, "decoder": None, "model": model}, ensure_ascii=False)


def wheel_normalizer(normalizers, chain):
    kind = {"N": normalizers.NFD, "L": normalizers.Lowercase, "S": normalizers.StripAccents}
    return normalizers.Sequence([kind[c]() for c in chain])


def char_isolating_file(chain):
    """a WordLevel file whose pre-tokenizer isolates every char and whose vocabulary knows none: one [UNK] per normalized char, its
    offsets the source range the reference aligns that char to (the strings hold no newline: `.` matches every char of them)"""
    return json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": sequence(chain),
                       "pre_tokenizer": {"type": "Split", "pattern": {"Regex": "."}, "behavior": "Isolated", "invert": False},
                       "post_processor": None, "decoder": None, "model": {"type": "WordLevel", "vocab": {"<unk>": 0}, "unk_token": "<unk>"}})


# bases whose members disagree most: two-step lowercase (U+0130), three pieces (U+0390, U+1F82), Hangul LV / LVT, a titlecase digraph,
# final sigma, sharp s, a precomposed letter whose base lowercases, Me and Mc marks as chars of their own
BASES = ["a", "E", "Z", " ", "\u00c9", "\u00e9", "\u0130", "\u0390", "\u1f82", "\ud55c", "\uac00", "\u01c5", "\u00df", "\u03a3", "\u1e9e", "\u212b", "\u0958",
         "\u4e2d", "\U0001d400", "\u0149", "\u01f0", "x"]
MARKS = ["\u0301", "\u0316", "\u0327", "\u0345", "\u0334", "\u0308", "\u0488", "\u0903", "\u093c", "\u094d", "\u3099", "\u05b0", "\u0651", "\u20dd", "\u1ab0"]


def seeded_strings(n, seed):
    """bases and marks, the marks in and out of canonical order"""
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


# ---- documents for the device --------------------------------------------------------------------------------------------------------
FILL = "ab cd ef gh "


def _filled(n):
    return (FILL * (n // len(FILL) + 1))[:n]


def straddle_docs(chars, big):
    """per char c: documents in which c ENDS at byte 16 and 64 (for the chars of `big`: and 4096) of the text (the document first in its
    batch) and in which it begins one byte before them (at 4095: every other char of `big`); c first and last in a document"""
    out = []
    for c in chars:
        n = len(c.encode("utf-8"))
        for edge in (16, 64):
            out.append(_filled(edge - n) + c + "z tail")
            out.append(_filled(edge - 1) + c + " tail")
        if c in big:
            out.append(_filled(4096 - n) + c + "z tail")
            if big.index(c) % 2 == 0:
                out.append(_filled(4095) + c + " tail")
        out.append(c + "start")
        out.append("end" + c)
        out.append(c)
    return out


CHANGING = ["\u00e9", "\u00c9", "\u0130", "\ud55c", "\uac00", "\u0390", "\u1f82", "\u0301", "\u0488"]
BIG = ["\u00e9", "\u0130", "\ud55c", "\u0301"]         # 2 -> 1 byte, 2 -> 3 bytes, 3 -> 9 bytes, 2 -> 0 bytes (by the chain)
RAW_TOKEN, NORM_TOKEN = "<raw>", "Caf\u00e9"


def edge_docs():
    """what every fixture encodes: the straddling documents, an empty one, documents and words that normalize to nothing, marks behind a
    raw added-token match and at a document's start, the normalized added token in several cases, and prose"""
    d = straddle_docs(CHANGING, BIG)
    d += ["", "\u0301", "\u0301\u0488", "\u00c1B \u0301 \u00c1b", "a \u0301\u0316 b", "\u0301 x", "x \u0301",
          RAW_TOKEN + "\u0301 x", "a" + RAW_TOKEN + "\u0301", "\u0301" + RAW_TOKEN, "E\u0301" + RAW_TOKEN + "\u0316\u0301e",
          "CAF\u00c9 au lait", "a caf\u00e9 b", "Cafe\u0301 CAFE\u0301", "xCaf\u00c9x", "\u0130stanbul I\u0307 i\u0307",
          "\ud55c\uad6d\uc5b4 \ubb38\uc7a5", "\u039f\u0394\u039f\u03a3 \u03c3\u03c2", "Stra\u00dfe STRASSE \u1e9e", "e\u0316\u0301 e\u0301\u0316",
          "\u0958 \u0915\u093c \u212b A\u030a", "MixedCase camelCaseWord HTTPServer's", "tabs\tand\nnewlines\r\n", "\u4e2d\u6587 \U0001f600 ok"]
    return d


def batch_docs(prose):
    """the fixture's batch: more than two workgroups of text (4,096 bytes each), a document count that is no multiple of 256"""
    d = edge_docs() + list(prose)
    while len(d) % 256 in (0, 255):
        d.append("pad\u00e9")
    return d


MARKS30 = "".join(chr(0x300 + (7 * k) % 0x30) for k in range(30))
MARKS60 = "".join(chr(0x300 + (7 * k) % 0x30) for k in range(60))


def out_of_order_docs():
    """NFD stays in the text: marks out of canonical order (their offsets go by position), across words, behind a char that decomposes
    into a base and a mark of its own, at a document's start, and thirty of them behind one base"""
    return ["e\u0301\u0316 x", "\u00e9\u0316\u0327 \u00c9\u0327\u0316", "a\u0345\u0301\u0316b", "\u0316\u0301 \u0301\u0316", "\u0301\u0316start",
            "\u1f82\u0316 \u0390\u0327", "\u0130\u0316 I\u0316\u0307", "\ud55c\u0301\u0316", "q\u0f73\u0f71 \u0344\u0316", "A" + MARKS30 + " b",
            "x\u0958\u0316\u0301y \u212b\u0316"]
