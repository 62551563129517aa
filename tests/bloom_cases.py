"""Documents for BLOOM's Sequence[Split(Regex " ?[^(\\s|[.,!?…。，、।۔،])]+", Isolated), ByteLevel(use_regex=false)]
(csrc/pretok_bloom_core.hpp), shared by the fixture generator (tools/make_golden_bloom.py) and the tests (tests/test_bloom.py,
tests/test_bloom_gpu.py): the smallest shapes at which the lane kernel (one lane per 64-byte mask word, 64 lanes a wavefront, 256 lanes =
16384 bytes a workgroup) can go wrong."""
import random

from oracle import synth

NAME = "bloom_bpe"
PATTERN = " ?[^(\\s|[.,!?…。，、।۔،])]+"
BOS, EOS, PAD, USER, ASSISTANT = "<s>", "</s>", "<pad>", "<|user|>", "<|assistant|>"

# the 39 scalars the pattern's class leaves out: Oniguruma's \s (25) and fourteen punctuation marks
ONIG_S = [chr(c) for c in list(range(0x09, 0x0E)) + [0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]]
PUNCT = list("!(),.?|") + [chr(c) for c in (0x060C, 0x06D4, 0x0964, 0x2026, 0x3001, 0x3002, 0xFF0C)]
X39 = ONIG_S + PUNCT
assert len(X39) == len(set(X39)) == 39
X2, X3 = ["\u0085", "\u00a0"], ["。", "，"]            # X chars of two and of three bytes

# the issue's examples: text -> pieces (␠ written as a space)
TABLE = [
    ("a  b   c", ["a", " ", " b", "  ", " c"]),
    ("a..  b", ["a", ".. ", " b"]),
    ("x ", ["x", " "]),
    ("(|)[]", ["(|)", "[]"]),
    (" [x]", [" [x]"]),
]

# the random strings' alphabet: all 39, class chars of 1..4 bytes (with `[` and `]`, a zero-width space and a combining mark), many spaces
ALPHABET = X39 + list("ab[]é中😀0'") + ["\u200b", "\u0301"] + [" "] * 12
EDGES = (64, 4096, 16384)                                          # a mask word, a wavefront, a workgroup


def random_strings(n, seed, lo=0, hi=48, alphabet=None):
    rng = random.Random(seed)
    alphabet = alphabet or ALPHABET
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def nbytes(s):
    return len(s.encode("utf-8"))


def filler(n):
    """n bytes that are few tokens and end in letters (16 KB of one letter would be 16 K tokens in the vectors)"""
    return "the " * ((n - 8) // 4) + "x" * (n - 4 * ((n - 8) // 4)) if n >= 12 else "x" * n


def around(edge, off, item, tail="y z"):
    """`item` with its first byte at byte edge + off, behind letters"""
    return filler(edge + off) + item + tail


def edge_items():
    """what is placed around every edge: each of the 39, a space followed by a class char, a class char followed by an X char"""
    return X39 + [" a", "a.", " é", "中。", "  b", ". a"]


def constructed_docs(edge):
    """every item at every offset -8..+8 around byte `edge`; X chars of two and three bytes at every split across it: between letters,
    between spaces, behind a space and in front of a class char, doubled"""
    docs = [around(edge, off, item) for item in edge_items() for off in range(-8, 9)]
    for ch in X2 + X3:
        w = nbytes(ch)
        for k in range(0, w + 1):                       # k of the char's bytes in front of the edge
            docs += [filler(edge - k) + ch + "y z", filler(edge - k - 1) + " " + ch + " y", filler(edge - k - 1) + " " + ch + "y", filler(edge - k - 1) + "." + ch + ch + "中"]
    return docs


def short_docs():
    docs = [t for t, _ in TABLE]
    docs += ["", " ", "  ", "a", ".", "a ", " a", "  a", "a  ", ". ", " .", "a.", ".a", "a .", "a. ", "a . b", "\n", "a\nb", "a \nb", "a\n b", "\t\t x", "[a] (b) |c|",
             "Hello, world! How are you?", "中文。日本語、テスト，ok", "आप कैसे हैं। ठीक", "یہ ہے۔ اور، بس", "wait… what", "a\u00a0b\u0085c\u3000d", "e\u0301 x\u200by", "😀 😀! 😀"]
    docs += X39 + ["a" + c + "a" for c in X39] + [" " + c + " " for c in X39] + [c + "a" for c in X39] + ["a " + c for c in X39]
    for n in (0, 1, 63, 64, 65, 127, 128, 129):         # text lengths around one and two mask words
        docs += ["a" * n, " " * n, "." * n, ("ab ." * 40)[:n], (" a" * 70)[:n], ("a " * 70)[:n], _fit("é。 ", n)]
    docs += [USER + "hi there." + ASSISTANT + " ok, fine " + EOS, "a " + USER + "b", "a" + USER + " b", "x. " + EOS + " y", BOS + "a", " " + USER + " ", USER + USER, "a " + EOS]
    return docs


def batches():
    """batches whose documents sit at other bytes than 0: a space as a document's last byte with a class char opening the next one, empty
    documents between them"""
    return [["x ", "y", "", " ", "z"], ["", "", "a b"], ["a ", "", "b", " ", "", ".", "c"], ["x" * 63 + " ", "y" * 63 + " ", "z"], ["x" * 62 + " ", "。y", " " * 9 + "a"],
            [" ", "a", " ", " a", "a ", ".", " ."], ["x" * 61 + "。", "。y", "a\u0085", "\u0085b"], ["", ""], ["a" * 64, "b" * 64, " " * 64, "c"]]


# ---- the device's edge documents: 16384 + 72 bytes each, one per edge family ------------------------------------------------------------

def _fit(unit, n):
    """n bytes of `unit` repeated, cut at a char edge and filled up with letters"""
    s = unit * (n // max(1, nbytes(unit)) + 2)
    b = s.encode("utf-8")[:n].decode("utf-8", "ignore")
    return b + "x" * (n - nbytes(b))


FAMILIES = {
    "the_39": "a" + "a".join(X39) + "b",
    "space_class": "a b  c   d    e é  中 ",
    "class_x": "ab.cd,e!f(g)h?i|j。k，l…m।n",
    "wide2": "a\u0085b\u00a0 \u0085 \u00a0c",
    "wide3": "a。 ，b\u3000 、",
    "brackets": "[a] (b) [ ] ( ) |[|]",
    "mixed": None,
}


def device_edge_doc(family):
    """one document of 16384 + 72 bytes: 36 bytes of the family's pattern on either side of the word edges 64 and 128, the wavefront edge
    4096 and the workgroup edge 16384 (a char of the wide families straddling each of them), filler between"""
    unit = FAMILIES[family] or "".join(random_strings(40, seed=77))
    strad = {"wide2": "\u00a0", "wide3": "，"}.get(family)

    def pat(n_front, n_back, k):
        if not strad:
            return _fit(unit, n_front + n_back)
        return _fit(unit, n_front - k) + strad + _fit(unit[1:] + unit[:1], n_back - (nbytes(strad) - k))
    doc = pat(64, 0, 1) + pat(64, 36, 1)
    doc += filler(4096 - 36 - nbytes(doc)) + pat(36, 36, 2 if family == "wide3" else 1)
    doc += filler(16384 - 36 - nbytes(doc)) + pat(36, 72, 1)
    assert nbytes(doc) == 16384 + 72, (family, nbytes(doc))
    return doc


def device_edge_docs():
    return [device_edge_doc(f) for f in FAMILIES]


def mixed_text(n_bytes, seed):
    """about n_bytes of prose with this rule's own trouble sprinkled in"""
    rng = random.Random(seed)
    lines = [ln for k in range(n_bytes // 12000 + 1) for ln in synth.gen_lines(300, text_seed=seed + 1000 * k)]
    extra = ["...", " . ", "  ", "   x", "(a|b)", "[1, 2]", "中文。", "、，", "… ", "\u00a0", "\u0085\u0085", " \u3000 ", "!?", "e\u0301", "\u200b", "😀", "\n\n", "\t", " ", ". "]
    parts, size = [], 0
    for ln in lines:
        parts.append(ln)
        parts.append(rng.choice(extra) if rng.random() < 0.6 else " ")
        size += nbytes(parts[-2]) + nbytes(parts[-1])
        if size >= n_bytes:
            break
    return "".join(parts)


def big_doc():
    """one document of about 70 KB: several workgroups of the lane kernel"""
    return mixed_text(70000, seed=23)
