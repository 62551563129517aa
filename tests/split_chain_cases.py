"""Documents for the chained Split pre-tokenizer of DeepSeek-V3 / R1 (csrc/pretok_ds3_core.hpp), shared by the fixture generator
(tools/make_golden_split_chain.py) and the tests (tests/test_split_chain.py, tests/test_split_chain_gpu.py): the smallest shapes at which
the lane kernel (48 bytes a lane inside a 64-byte window, 64-byte mask words, 256 lanes a workgroup) and the sequential matcher behind it
can go wrong."""
import random

from oracle import synth

BOS, EOS, USER, ASSISTANT, PAD = "<｜begin▁of▁sentence｜>", "<｜end▁of▁sentence｜>", "<｜User｜>", "<｜Assistant｜>", "<｜▁pad▁｜>"

# what the issue's table of chain versus alternation lists, and the facts read off it
TABLE = ["a  1", "  中", "中文abcかな1", "a‍b \x01\x02 c", "x .b ..b a.b._c"]

# one representative of each class the rule tells apart: ASCII letter, non-ASCII letter, mark, digit, non-ASCII digit, space, tab, LF, ASCII
# punctuation of the first alternative's class, a symbol outside it, a char of the CJK class, a format char
ALPHABET = ["a", "é", "́", "1", "٣", " ", "\t", "\n", ".", "€", "中", "‍"]
# (what the exhaustive strings cannot hold for their number: CR, a control, a 4-byte letter / symbol / digit, CJK-class chars that are a mark,
# a symbol, punctuation, unassigned; U+3000 and U+0085 whitespace; an upper-case letter; the apostrophe)
WIDE = ALPHABET + ["\r", "\x01", "\U00010400", "\U0001F601", "\U0001D7D8", "゙", "゛", "・", "぀", "か", "　", "\x85", "Z", "'", "!", "ab", "  "]

RUN_KINDS = {"letter": "a", "wide letter": "é", "mark": "́", "digit": "7", "wide digit": "٣", "space": " ", "newline": "\n", "punct": "!",
             "symbol": "€", "cjk": "中", "format": "‍", "control": "\x01"}


def window_edge_runs():
    """runs of each kind of length 1..20 ending exactly at, one before and one after a window edge (48 bytes a lane; the byte-64 mask-word
    edge rides along), in front of and behind other text"""
    out = []
    for edge in (48, 64, 96):
        for ch in RUN_KINDS.values():
            w = len(ch.encode("utf-8"))
            for n in range(1, 21):
                for end in (edge - 1, edge, edge + 1):
                    lead = end - n * w
                    if lead < 1:
                        continue
                    out.append("x" * (lead - 1) + " " + ch * n + "y z")
                    out.append("." * lead + ch * n)
    return out


def random_strings(n, seed, lo=40, hi=200, alphabet=None):
    rng = random.Random(seed)
    alphabet = alphabet or ALPHABET
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def mixed_text(n_bytes, seed):
    """about n_bytes of prose with everything else sprinkled in: digit runs, CJK runs, indentation, punctuation in front of letters,
    controls, marks"""
    rng = random.Random(seed)
    # (300 lines a call: the SIMT emulation's environment shrinks larger requests, and the vectors hold this text as it is here)
    lines = [ln for k in range(n_bytes // 12000 + 1) for ln in synth.gen_lines(300, text_seed=seed + 1000 * k)]
    extra = ["12345678", "3.14159", "中文かなカナ", " 中 ", "\n\n    ", "\t\t", "!important", "(see", "#tag", "x\x01\x02y", "café", "naïve", "€100", "  ", "２０２４",
             "a‍b", "...\n", " !!\r\n", "über", "\U0001F601\U0001F601", "١٢٣٤"]
    parts, size = [], 0
    for ln in lines:
        parts.append(ln)
        parts.append(rng.choice(extra) if rng.random() < 0.5 else " ")
        size += len(parts[-2].encode("utf-8")) + len(parts[-1].encode("utf-8"))
        if size >= n_bytes:
            break
    return "".join(parts)


def exact_length(n):
    """a document of exactly n bytes of mixed text"""
    unit, out, size, i = "ab 12 中. é\n", [], 0, 0
    while size + len(unit[i % len(unit)].encode("utf-8")) <= n:
        out.append(unit[i % len(unit)])
        size += len(out[-1].encode("utf-8"))
        i += 1
    return "".join(out) + "x" * (n - size)


def edge_docs():
    docs = list(TABLE)
    docs += ["", "a", "Z", "1", " ", "\t", "\n", "\r", ".", "$", "\x01", "é", "́", "٣", "中", "か", "・", "‍", "€", "\U0001F601", "\U00010400"]
    docs += [exact_length(n) for n in (47, 48, 49, 63, 64, 65)]
    for k in range(1, 8):                               # a digit run of 1..7 across a lane's edge and a mask word's edge
        for edge in (48, 64):
            docs.append("x" * (edge - (k + 1) // 2) + "1" * k + " a")
            docs.append("y " * ((edge - 1) // 2) + ("" if edge % 2 else " ") + "9" * k)
    for gap in (1, 3, 9):                               # a whitespace run that ends at a digit, a CJK char, the document's end, an added token
        for lead in (1, 46, 62):
            sp = " " * gap
            docs += ["a" * lead + sp + "1", "a" * lead + sp + "中", "a" * lead + sp, "a" * lead + sp + USER + "b", "a" * lead + "\n" + sp + "1"]
    for lead in (45, 46, 47, 61, 62, 63):               # a 3- and a 4-byte char split across two windows / mask words
        docs += ["x" * lead + "中x", "x" * lead + "\U0001F601 y", "x" * lead + "٣٣", "x" * lead + "́a"]
    for lead in (44, 46, 60, 62):                       # a stretch no alternative matches, across a window's edge
        docs += ["x" * lead + " \x01\x02\x03\x04\x05\x06 y", "x" * lead + "\x01\x02\x03\x04\x05\x06y", "x" * lead + "‍‍‍‍ z"]
    docs += ["!abcé d", "か゛か", "12345٣٣4", ".\n.b", "á ́b", "\x01\x02c", "!ab\n", "a . \n\n  b", "x" * 40 + "!abcdefghijklmnopé", "x" * 41 + " (abcdefghijklmnopqrstuvwxyzé",
             "Universität Zürich", "x" * 36 + " Universität", USER + "Hello 123 中文" + ASSISTANT + "  ok" + EOS, BOS + "x", "a" + USER, USER, USER + USER + "1234" + USER + " ",
             "tail  " + EOS + "  head", "1" * 100, " " * 80 + "x", "中" * 40 + "1" * 5 + "か" * 30, "\n" * 70, "." * 130 + "\n\n"]
    return docs


def big_doc():
    """one document of about 70 KB: several workgroups of the lane kernel, and the flagged-document list"""
    return mixed_text(70000, seed=17)


def short_batch(flagged=True):
    """a few hundred short documents; with `flagged` a handful the lane kernel cannot decide by itself (long digit / whitespace runs)"""
    docs = [d[:60] for d in synth.gen_lines(300, text_seed=23)]
    if flagged:
        for k, d in ((3, "1" * 90), (57, "x" + " " * 120 + "y"), (58, "7" * 64), (199, "\n" * 100 + "a"), (299, "abc " + "9" * 75 + " def")):
            docs[k] = d
    return docs


def plain_batch():
    """documents no lane leaves a byte of undecided: the sequential matcher's list is empty"""
    return ["ab cd", "x.y", "hello world", "中文 ok", "one 12 two", ""] * 20
