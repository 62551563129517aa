"""Seeded cases of the Precompiled normalizer in front of Unigram (XLM-R / T5 layout): a double-array builder for synthetic charsmaps (the
reference wheel accepts its output), the two charsmaps, the tokenizer.json files built around them, and the documents whose hard places are
byte positions -- clusters of 5, 6 and 7 bytes at lane, word and workgroup edges, removals at piece starts, documents that become nothing.
tools/make_golden_precompiled.py writes the fixtures from here with the wheel; the tests read them back and compare."""
import base64
import functools
import json
import random
import struct
import unicodedata

MS = "▁"
NAMES = ["precompiled_xlmr", "precompiled_ms"]
ZWJ = "\u200d"


# ---- the blob --------------------------------------------------------------------------------------------------------------------------
def build_charsmap(mapping, pad=256):
    """{key: replacement} -> the precompiled_charsmap bytes: u32 trie size, the darts-clone double array, NUL-terminated replacements"""
    rep, where = bytearray(), {}
    for v in sorted(set(mapping.values())):
        where[v] = len(rep)
        rep += v.encode("utf-8") + b"\0"
    trie = {}
    for k, v in mapping.items():
        node = trie
        for b in k.encode("utf-8"):
            node = node.setdefault(b, {})
        node[0] = where[v]                                   # label 0: the leaf
    units, used, bases = [0] * pad, {0}, set()
    todo = [(0, trie)]
    while todo:
        at, node = todo.pop()
        base = 1
        while base in bases or any((base ^ l) in used for l in node):
            base += 1
        bases.add(base)
        while len(units) <= base + 256:
            units += [0] * pad
        assert (at ^ base) < (1 << 21)
        units[at] |= (at ^ base) << 10
        for l, child in node.items():
            used.add(base ^ l)
            if l == 0:
                units[base] = 0x80000000 | child
                units[at] |= 1 << 8                          # has_leaf
            else:
                units[base ^ l] = l
                todo.append((base ^ l, child))
    units = units[:(max(used) // pad + 1) * pad]
    return struct.pack("<I", 4 * len(units)) + struct.pack("<%dI" % len(units), *units) + bytes(rep)


def adversarial_map():
    """prefix keys, multi-char keys, empty replacements, expansions, a space and a U+2581 in a replacement, keys of 1..4 bytes"""
    return {"a": "b", "ab": "Q", "\r\n": "\n", "e\u0301": "\u00e9", "\u00e9": "\u00e9", "\x1e": "", "\u200b": "", "\ufeff": "", "\u2122": "TM", "\ufb03": "ffi",
            "\t": " ", "\u00bd": "1 2", "\u2022": MS, "\u00a9": "(c)", "\U0001f600": ":)", "\U0001f1e6": "A", "\u0600": "", "\u0e33": "\u0e4d\u0e32",
            "z\u0301\u0302": "Z", "\u3000": " ", "\ufdfa": unicodedata.normalize("NFKC", "\ufdfa"), "\u0915": "k", "\u1100": "g"}


def nmt_nfkc_like_map(limit=3000, seed=5):
    """a few thousand scalars with NFKC(c) != c, base + mark -> composed, controls to "" or " ", Unicode spaces to " ", U+FEFF / U+200B removed"""
    rng = random.Random(seed)
    m = {}
    cands = [c for c in range(0xA0, 0x30000) if not 0xD800 <= c < 0xE000 and unicodedata.normalize("NFKC", chr(c)) != chr(c)
             and "\0" not in unicodedata.normalize("NFKC", chr(c))]
    for c in rng.sample(cands, limit) + [0xFB03, 0x2122, 0xFDFA, 0xBD, 0xFF21, 0x3300]:
        m[chr(c)] = unicodedata.normalize("NFKC", chr(c))
    for c in cands:
        d = unicodedata.normalize("NFD", chr(c))
        if len(d) == 2 and unicodedata.normalize("NFC", d) == chr(c) and rng.random() < 0.5:
            m[d] = chr(c)
    for c in list(range(1, 9)) + list(range(0xE, 0x20)) + [0x7F]:
        m[chr(c)] = ""
    for c in (0x9, 0xA, 0xC, 0xD, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000, 0xA0) + tuple(range(0x2000, 0x200B)):
        m[chr(c)] = " "
    m["\ufeff"] = m["\u200b"] = ""
    return m


# ---- the tokenizers --------------------------------------------------------------------------------------------------------------------
def _vocab(seed):
    rng = random.Random(seed)
    pieces = ["<unk>", "<s>", "</s>", MS]
    alphabet = "abcdefghijklmnopqrstuvwxyzQZTMk1 2()\u00e9\u0e4d\u0e32:)"
    seen = set(pieces)
    for ch in sorted(set(alphabet.replace(" ", ""))) + ["\u0635", "\u0644", "\u0649", "f", "i", "\u4e2d", "\u6587", "\uac00"]:
        for p in (ch, MS + ch):
            if p not in seen:
                seen.add(p)
                pieces.append(p)
    while len(pieces) < 900:
        w = "".join(rng.choice("abcdefghijklmnoprstuw") for _ in range(rng.randint(2, 6)))
        p = (MS if rng.random() < 0.5 else "") + w
        if p not in seen:
            seen.add(p)
            pieces.append(p)
    return [[p, 0.0 if i < 3 else -round(rng.uniform(1.0, 14.0), 6)] for i, p in enumerate(pieces)]


@functools.lru_cache(maxsize=None)
def tokenizer_json(name):
    """precompiled_xlmr: the layout of xlm-roberta-base (Sequence[Precompiled, Replace " {2,}"] + Sequence[WhitespaceSplit, Metaspace]), the
    nmt_nfkc-like charsmap, byte_fallback, specials and a template; precompiled_ms: Precompiled alone in front of bare Metaspace, the
    adversarial charsmap, an lstrip / rstrip special"""
    xlmr = name == "precompiled_xlmr"
    vocab = _vocab(3 if xlmr else 4)
    if xlmr:
        vocab += [["<0x%02X>" % b, -20.0] for b in range(256)]
    cm = base64.b64encode(build_charsmap(nmt_nfkc_like_map() if xlmr else adversarial_map())).decode()
    pc = {"type": "Precompiled", "precompiled_charsmap": cm}
    ms = {"type": "Metaspace", "replacement": MS, "prepend_scheme": "always", "split": True}
    n = len(vocab)
    added = [{"id": 1, "content": "<s>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True},
             {"id": 2, "content": "</s>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True},
             {"id": n, "content": "<mask>", "single_word": False, "lstrip": True, "rstrip": not xlmr, "normalized": False, "special": True}]
    tpl = {"type": "TemplateProcessing",
           "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}}],
           "pair": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}},
                    {"SpecialToken": {"id": "</s>", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}}],
           "special_tokens": {"<s>": {"id": "<s>", "ids": [1], "tokens": ["<s>"]}, "</s>": {"id": "</s>", "ids": [2], "tokens": ["</s>"]}}}
    return json.dumps({
        "version": "1.0", "truncation": None, "padding": None, "added_tokens": added,
        "normalizer": {"type": "Sequence", "normalizers": [pc, {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}]} if xlmr else pc,
        "pre_tokenizer": {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, ms]} if xlmr else ms,
        "post_processor": tpl, "decoder": None,
        "model": {"type": "Unigram", "unk_id": 0, "vocab": vocab, "byte_fallback": xlmr}}, ensure_ascii=False)


# ---- the documents ---------------------------------------------------------------------------------------------------------------------
def clusters():
    """clusters of exactly 5, 6 and 7 bytes of each composition, and the ones the rules are about"""
    return ["a\u0301\u0302", "\u00e9\u3099", "\u3042\u0301", "a\U000e0101", "\u00a9" + ZWJ + "\u00a9", "\u00a9" + ZWJ, "\u0600a", "\u0600\u00e9", "\r\n", "\r", "\n\r",
            "a\u0301\u0302\u0303", "e\u0301", "\u00e9\u0302", "z\u0301\u0302", "ab", "a", "e\u0301\u0302", "\u2122\u0301", "\ufb03\u0301", "\u0e01\u0e33",
            "\U0001f600" + ZWJ + "\U0001f600", "\U0001f1e6\U0001f1e7", "\U0001f1e6\U0001f1e7\U0001f1e8", "\u0915\u094d\u0937", "\u1100\u1161\u11a8", "\uac00\u11a8",
            "\u200b", "\ufeff", "\x1e\x1e", "\u0600", "\u00bd", "\u2022x", "x\u2022y", "\ufdfa", "\u00a9\u0301" + ZWJ + "\u00a9", "a" + ZWJ + "\u00a9"]


def table_rows():
    """the inputs of the issue's alignment table"""
    return ["\x1exy", "\x1e\x1exyz \ufb03", "\ufb03\x1ex", "x\x1e\x1ey", "a  \u2122\x1ea\t \u00e9"]


def prose(rng, n_bytes, odd=0.05):
    words, size = [], 0
    cl = clusters()
    while size < n_bytes:
        r = rng.random()
        if r < odd:
            w = rng.choice(cl)
        elif r < odd + 0.04:
            w = rng.choice(["\u4e2d\u6587", "caf\u00e9", "nai\u0308ve", "\uff21\uff22", "\u2122", "<mask>", "\ufb03", "\uac00\uac01", "x\u200by", "\u00a0", "\t", "\n"])
        else:
            w = "".join(rng.choice("abcdefghijklmnoprstuw") for _ in range(rng.randint(1, 9)))
        words.append(w)
        size += len(w.encode()) + 1
    return " ".join(words)


def split_clusters():
    """every cluster of two chars or more cut behind its first char: (what ends one document, what begins the next)"""
    return [(c[0], c[1:]) for c in clusters() if len(c) > 1]


def edge_documents():
    """every cluster first and last in a document, straddling a 16-byte lane, a 64-byte word and a 4,096-byte workgroup edge (the document
    is first in its batch, so the cluster sits at exactly that byte), next to an added token, behind a removal"""
    docs = list(table_rows())
    for k, c in enumerate(clusters()):
        docs += [c, c + "x y", "x y" + c, "<mask>" + c, c + "<mask>" + c, "\ufeff" + c, " " + c + " "]
        for edge in (16, 64, 4096):
            for back in ((1, 2, 3) if edge < 4096 else (1 + k % 3,)):
                fill = edge - back
                docs.append(("ab cd " * (fill // 6 + 1))[:fill - 1] + "x" + c + " tail" if edge < 4096 else ("lorem ipsum " * 400)[:fill - 1] + "x" + c + " tail")
    # a cluster across a document edge, and across an added token: the edge is a text boundary, the rest opens a piece of its own
    for a, b in split_clusters():
        docs += ["x y" + a, b + " z", a + "<mask>" + b, "q" * 14 + a + "<mask>" + b]
    docs += ["\ufeffxy z", "\x1e", "\u200b\ufeff", " \t ", "", "<mask>\ufeffx", "a<mask>\x1e\x1ey z", "x <mask> y", "<s>\u200bq</s>", "▁x ▁▁y a▁b"]
    return docs


def corpus():
    rng = random.Random(17)
    docs = edge_documents()
    docs += ["", "", ""] + [rng.choice("abxyz\x1e\u00e9\u4e2d \u2122") for _ in range(40)]
    docs += [prose(rng, rng.randint(5, 300)) for _ in range(120)]
    docs.append(prose(rng, 20000, odd=0.08))
    return docs


def pairs():
    rng = random.Random(23)
    e = edge_documents()
    return [(rng.choice(e), prose(rng, rng.randint(5, 80))) for _ in range(40)] + [(prose(rng, 60), rng.choice(e)) for _ in range(40)]
