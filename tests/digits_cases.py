"""Documents for Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family (csrc/pretok_digits_core.hpp), shared by the fixture
generator (tools/make_golden_digits.py) and the tests (tests/test_digits.py, tests/test_digits_gpu.py): the smallest shapes at which the
lane kernel (one lane per 64-byte mask word, 64 lanes a wavefront, 256 lanes = 16384 bytes a workgroup) can go wrong."""
import random

from oracle import synth

BOS, EOS, PAD, USER, ASSISTANT = "<|begin|>", "<|endoftext|>", "<|pad|>", "<|user|>", "<|assistant|>"
NAMES = ("digits_individual", "digits_contiguous")

# the issue's table: text -> pre-tokens with individual_digits true / false (byte-level alphabet: Ġ = space, Ċ = LF)
TABLE = [
    ("abc 123 de", ["abc", "Ġ", "1", "2", "3", "Ġde"], ["abc", "Ġ", "123", "Ġde"]),
    ("a  1", ["a", "ĠĠ", "1"], ["a", "ĠĠ", "1"]),
    ("x=12.5e3\n\n 7", ["x", "=", "1", "2", ".", "5", "e", "3", "ĊĊĠ", "7"], ["x", "=", "12", ".", "5", "e", "3", "ĊĊĠ", "7"]),
    ("it's 3pm", ["it", "'s", "Ġ", "3", "pm"], ["it", "'s", "Ġ", "3", "pm"]),
    ("Ⅷ and ٣٤ ½", None, None),      # (checked by offsets: the byte-level spelling of the multi-byte chars says nothing)
]
TABLE_WIDE_INDIVIDUAL = ["Ⅷ", " and", " ", "٣", "٤", " ", "½"]

# numeric chars of 2, 3, 3 and 4 bytes (½ is 2 bytes, ٣ 2, Ⅷ 3, U+1D7CE 4), and the two classes' difference: numeric for Rust, not \p{N}
# for the regex engine (4 bytes each)
NUM2, NUM2B, NUM3, NUM4 = "٣", "½", "Ⅷ", "\U0001D7CE"
RUST_ONLY = ["\U00011DE0", "\U00016FF4"]
WIDE_NUMERIC = [NUM2, NUM2B, NUM3, NUM4] + RUST_ONLY

# the exhaustive strings' alphabet (the issue's): letter, space, LF, digit, apostrophe, s, a 2-byte digit, a 4-byte digit, a Rust-only numeric
ALPHABET = ["a", " ", "\n", "1", "'", "s", "٣", "\U0001D7CE", "\U00011DE0"]
WIDE = ALPHABET + ["é", "\t", "\r", ".", "€", "中", "Ⅷ", "½", "\U00016FF4", "\U0001F601", "t", "re", "ll", "9", "  ", "Z", " ", "　", "́"]


def random_strings(n, seed, lo=40, hi=200, alphabet=None):
    rng = random.Random(seed)
    alphabet = alphabet or ALPHABET
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def mixed_text(n_bytes, seed):
    """about n_bytes of prose with code-like digits sprinkled in: literals, versions, wide digits, indentation, contractions next to digits"""
    rng = random.Random(seed)
    lines = [ln for k in range(n_bytes // 12000 + 1) for ln in synth.gen_lines(300, text_seed=seed + 1000 * k)]
    extra = ["12345678", "3.14159", "0x1F", "v2.10.3", " 42 ", "\n\n    7", "\t\t1", "x[10]=y[2];", "1e-9", "٣٤٥", "Ⅷ", "½", "\U0001D7CE\U0001D7CF", "1\U00011DE02",
             "\U00016FF4", "it's 3pm", "1's", "'s1", "  9", "２０２４", "café 5", "€100", "a1b2c3", "\U0001F601" + "7", " ", "\n"]
    parts, size = [], 0
    for ln in lines:
        parts.append(ln)
        parts.append(rng.choice(extra) if rng.random() < 0.6 else " ")
        size += len(parts[-2].encode("utf-8")) + len(parts[-1].encode("utf-8"))
        if size >= n_bytes:
            break
    return "".join(parts)


def filler(n):
    """n bytes that are few tokens and end in letters (16 KB of one letter would be 16 K tokens in the vectors)"""
    return "the " * ((n - 8) // 4) + "x" * (n - 4 * ((n - 8) // 4)) if n >= 12 else "x" * n


def straddles(edge, chars=None, shapes=(0, 1, 2, 3)):
    """a numeric char of 2, 3 and 4 bytes at every split across byte `edge` (and wholly on either side of it): between letters, between
    spaces, inside a run of digits, doubled in front of a contraction"""
    out = []
    for ch in chars or WIDE_NUMERIC:
        w = len(ch.encode("utf-8"))
        for k in range(0, w + 1):                       # k of the char's bytes in front of the edge
            lead = edge - k
            shaped = [filler(lead) + ch + "y z", filler(lead - 1) + " " + ch + " y", filler(lead - 2) + "12" + ch + "34", filler(lead - 2) + "  " + ch + ch + "'s"]
            out += [shaped[q] for q in shapes]
    return out


def edge_docs():
    docs = [t for t, _, _ in TABLE]
    docs += ["", "1", "a", " ", "\n", "12", "1a", "a1", " 1", "1 ", NUM2, NUM3, NUM2B, NUM4] + RUST_ONLY
    for at in (0, 63, 64):                              # a numeric char at bytes 0, 63 and 64 of a mask word
        for ch in ["7", NUM2, NUM3, NUM4, RUST_ONLY[0]]:
            docs += ["x" * at + ch + "y", " " * at + ch + " ", "x" * at + ch]
    docs += straddles(64) + straddles(128)
    docs += straddles(16384, chars=[NUM2, NUM2B, NUM3, NUM4], shapes=(0, 2))      # the workgroup's edge (and, at 4096, a wavefront's)
    docs += straddles(16384, chars=RUST_ONLY[:1], shapes=(2,)) + straddles(4096, chars=[NUM3, NUM4], shapes=(0,))
    for gap in (1, 2, 9):                               # a whitespace run in front of a digit, straddling a word edge
        for lead in range(64 - gap - 1, 65):
            if lead >= 1:
                docs += ["a" * lead + " " * gap + "1", "a" * lead + "\n" * gap + NUM2 + "b", "a" * lead + " " * gap + USER + "1"]
    docs += ["1's", "'s1", "it's 3pm", "1't", "1're 2've 3'll", "'re1", "1'd2'm3", "x" * 61 + "1's", "x" * 62 + "1're", "x" * 63 + "'ll1", "x" * 60 + "9'ves"]
    docs += ["1abc", "abc1", "1", "9 z 9", "7" + USER, USER + "7", "a" + USER + "12" + ASSISTANT + "34" + EOS, BOS + "1", "12" + EOS + "34", USER + USER + "5" + USER,
             "1" + EOS, " 1" + USER + " 2"]
    docs += ["1" * 200, "x" + "1" * 200 + "y", " " + "٣" * 100, "12" + RUST_ONLY[0] + "34" + RUST_ONLY[1] + "56", RUST_ONLY[0] + "1", "1" + RUST_ONLY[1], "a" + RUST_ONLY[0] + RUST_ONLY[1] + "b",
             "x=12.5e3", "0x1F", "v2.10.3-rc1", "arr[10][20] = 3;", "  1  22  333", "1\n2\r\n3\t4", "½ cup", "x²+y³", "②③", "１２３", "१२३ ४", "a 1", "1　2"]
    return docs


def batches():
    """batches whose documents sit at other bytes than 0: empty documents between digit documents, digits first and last in neighbouring
    documents"""
    return [["1", "", "2", "", "", "34", ""], ["", "", "7"], ["12", "34", "a5", "6b", NUM4, NUM4 + "1", "1" + NUM3], ["x" * 63 + "1", "2" + "y" * 63, "3"],
            ["x" * 62 + NUM3, NUM3 + "y", " " * 9 + "1"], [" ", "1", " ", " 1", "1 "]]


def big_doc():
    """one document of about 70 KB: several workgroups of the lane kernel"""
    return mixed_text(70000, seed=19)
