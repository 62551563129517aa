"""The CLIP layout -- Sequence[NFC, Replace(\\s+), Lowercase] + Sequence[Split(the CLIP pattern, Removed, inverted), ByteLevel] + byte-level BPE
with end_of_word_suffix "</w>" (csrc/pretok_clip_core.hpp, the NFC_LOWER mode of csrc/nfc_core.hpp, DevTables::byte_sfx) -- as a synthetic
file and the documents that go with it, shared by the fixture generator (tools/make_golden_clip.py) and the tests (tests/test_clip.py,
tests/test_clip_gpu.py): the smallest shapes at which the lane kernels (one lane per 64-byte mask word, 64 lanes a wavefront = 4,096
bytes, 256 lanes = 16,384 bytes a workgroup; the normalizer's 16-byte lanes) and the merge tiers (16 / 32 / 64 / 8,192 bytes) can go wrong."""
import json
import random

NAMES = ("clip_bpe", "clip_bpe_plain")          # the second: without the normalized added token (decode_batch is on the path there)
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
SUFFIX = "</w>"
PATTERN = "'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+"
NFC, LOWER = {"type": "NFC"}, {"type": "Lowercase"}
REPLACE = {"type": "Replace", "pattern": {"Regex": "\\s+"}, "content": " "}
SPLIT = {"type": "Split", "pattern": {"Regex": PATTERN}, "behavior": "Removed", "invert": True}
BYTELEVEL = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}

# chars the tests put at the edges: a contraction, an O run ending in ', a digit, a 4-byte char, a char that lowercases to two (U+0130)
DOTTED_I, EMOJI, ARABIC_3 = "İ", "\U0001f601", "٣"
EDGE_ATOMS = ["it's", "x're", "!!'", "7", EMOJI, DOTTED_I, ARABIC_3, "café", "Å"]
WHITESPACE = [" ", "\u00a0", "\u2003", "\u3000", "\t", "\n", "\r\n", "\u0085", "\u001c", "\u000b"]
ATOMS = ["the", "And", "ING", "it's", "IT'S", "'Re", "don't", "x'll", "12", "7", ARABIC_3, "!!", "!'s", "...", "café", "CAFÉ", DOTTED_I, "ǅ", "ß",
         "Σ", "ΑΣ", "中文", "́", "é", "ﬁ", "Å", "Å", SOT, SOT.upper(), EOT, EOT.upper(), EMOJI, "'", "''s", "a'", "_",
         "\u200b", "a", "I", "K", "ſ", "photo", "of", "a"] + WHITESPACE + [" ", " ", "  "]


def byte_alphabet():
    """the byte-level alphabet: chr of byte b's char, for b = 0..255 (pre_tokenizers/byte_level.rs bytes_char)"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def to_alphabet(word):
    al = byte_alphabet()
    return "".join(al[b] for b in word.encode("utf-8"))


# the words the merges are learned from (lower case: what the normalizer leaves), most frequent first
MERGE_WORDS = ["the", "and", "ing", "photo", "of", "a", "an", "in", "on", "'s", "'t", "'re", "'ll", "'ve", "it", "don", "café", "é", "!!", "!!!", "...", "!'", "''",
               "there", "other", "then", "thin", "king", "sing", "singing", "cat", "cats", "dog", "dogs", "house", "red", "re", "d", "s", "t", "ll", "ve", "photograph",
               "photographer", "landscape", "portrait", "painting", "of", "with", "without", "light", "lighting", "high", "quality", "detailed", "realistic", "style",
               "art", "artist", "by", "in", "at", "sunset", "sunrise", "mountain", "mountains", "river", "ocean", "city", "street", "night", "day", "blue", "green",
               "white", "black", "color", "colour", "colorful", "beautiful", "中", "文", "中文", EMOJI, "i̇", "å", "straße", "σ", "ασ",
               "k", "x", "é", "ﬁ", "abcdefghijklmnopqrstuvwxyz", "zzzzzzzz", "aaaaaaaaaaaaaaaa", "internationalization", "--", "->", "=>", "://", "http", "https",
               "www", ".com", "@", "#", "##", "$", "%", "&", "(", ")", "()", "[]", "{}", "\"", "\"\"", ",", ".", ";", ":", "?", "!", "_", "__"]


def build_vocab(n_merges=420):
    """256 byte chars, their 256 "</w>" forms, then greedy pair merges over MERGE_WORDS (weighted by their place): whole words, suffixed
    pieces, the two bytes of a 2-byte char, contractions and punctuation runs all merge"""
    al = byte_alphabet()
    vocab = {}
    for b in range(256):
        vocab[al[b]] = len(vocab)
    for b in range(256):
        vocab[al[b] + SUFFIX] = len(vocab)
    words = []
    for k, w in enumerate(MERGE_WORDS):
        syms = [al[b] for b in w.encode("utf-8")]
        syms[-1] += SUFFIX
        words.append((syms, len(MERGE_WORDS) - k))
    merges = []
    while len(merges) < n_merges:
        count = {}
        for syms, wt in words:
            for a, b in zip(syms, syms[1:]):
                count[(a, b)] = count.get((a, b), 0) + wt
        if not count:
            break
        (a, b), _ = max(count.items(), key=lambda kv: (kv[1], kv[0]))
        merges.append([a, b])
        vocab[a + b] = len(vocab)
        for syms, _ in words:
            i = 0
            while i + 1 < len(syms):
                if syms[i] == a and syms[i + 1] == b:
                    syms[i:i + 2] = [a + b]
                else:
                    i += 1
    return vocab, merges


def file_of(normalized_sot=True, normalizer=None, pre_tokenizer=None, model=None, **over):
    """the fixture file as a dict -> JSON; normalized_sot = False: the variant whose "<|startoftext|>" is normalized = false"""
    vocab, merges = build_vocab()
    vocab = dict(vocab)
    vocab[SOT] = len(vocab)
    vocab[EOT] = len(vocab)
    d = {"version": "1.0", "truncation": None, "padding": None,
         "added_tokens": [{"id": vocab[SOT], "content": SOT, "single_word": False, "lstrip": False, "rstrip": False, "normalized": normalized_sot, "special": True},
                          {"id": vocab[EOT], "content": EOT, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}],
         "normalizer": {"type": "Sequence", "normalizers": [NFC, REPLACE, LOWER]} if normalizer is None else normalizer,
         "pre_tokenizer": {"type": "Sequence", "pretokenizers": [SPLIT, BYTELEVEL]} if pre_tokenizer is None else pre_tokenizer,
         "post_processor": {"type": "RobertaProcessing", "sep": [EOT, vocab[EOT]], "cls": [SOT, vocab[SOT]], "trim_offsets": False, "add_prefix_space": False},
         "decoder": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": False, "use_regex": True},
         "model": {"type": "BPE", "dropout": None, "unk_token": EOT, "continuing_subword_prefix": "", "end_of_word_suffix": SUFFIX, "fuse_unk": False,
                   "byte_fallback": False, "ignore_merges": False, "vocab": vocab, "merges": merges}}
    if model:
        d["model"].update(model)
    d.update(over)
    return json.dumps(d, ensure_ascii=False)


def random_docs(n, seed, lo=0, hi=14, atoms=None):
    rng = random.Random(seed)
    atoms = atoms or ATOMS
    return ["".join(rng.choice(atoms) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def filler(n):
    """n bytes of lower-case words that are few tokens (16 KB of one letter would be 16 K tokens in the vectors) and end in a letter"""
    if n < 30:
        return "x" * n
    k = (n - 8) // 21
    return "internationalization " * k + "x" * (n - 21 * k)


def straddles(edge, atoms=None):
    """every atom at every split across byte `edge` (and wholly on either side of it), between letters and between spaces"""
    out = []
    for at in atoms or EDGE_ATOMS:
        w = len(at.encode("utf-8"))
        for k in range(0, w + 1):                          # k of the atom's bytes in front of the edge
            lead = edge - k
            out.append(filler(lead) + at + "y z")
            out.append(filler(lead - 1) + " " + at + " y")
    return out


def edge_docs():
    """each runs FIRST in a batch of its own, so the atom sits at exactly that byte"""
    docs = []
    for at in EDGE_ATOMS:                                   # first, last, alone in a document; as the last bytes of a batch
        docs += [at, at + " tail", "head " + at, "head" + at, at + "tail", " " + at + " "]
    docs += straddles(64) + straddles(128, atoms=EDGE_ATOMS[:6])
    docs += straddles(4096, atoms=EDGE_ATOMS[:6]) + straddles(16384, atoms=EDGE_ATOMS[:6])
    for at in EDGE_ATOMS[:6]:                               # ending at a lane's word, a wavefront's bytes, the workgroup's edge -- as the text's last bytes
        w = len(at.encode("utf-8"))
        docs += [filler(e - w - 1) + " " + at for e in (64, 128, 4096, 16384)]
        docs += [filler(e - w) + at for e in (64, 16384)]
    return docs


def run_docs():
    return ["1" * 300, "x" + "7" * 300 + "y", "'" * 300, "a" + "'" * 300 + "s", "'s" * 150, ARABIC_3 * 150,
            "ab" * 4500 + "a",                                # a 9 KB letter run: the huge merge tier, its last byte suffixed
            " ", "   ", "\n\t \u00a0\u3000", "\u0085\u001c\u000b", "", "\u200b", " \u200b "]


def last_byte_docs():
    """words whose last byte decides the id: a one-byte word is "a</w>", never "a"; a word that is exactly an entry minus its suffix"""
    return ["a", "a a", "aa", "a aa a", "the", "the the", "thethe", "th", "t h e", "photo", "photograph", "photographs", "é", "café", "cafés", "!", "!!", "!!!", "!!!!",
            "d", "re", "'re", "'red", "''s", "!'s", "it's", "don't", "i'll", "they've", "i'm", "he'd", "'s", "x's's", "'S", "IT'S", "x'", "x''", "'", "a'b", "1's", "'1",
            "abcdefghijklmnopqrstuvwxyz", "abcdefghijklmnop", "abcdefghijklmnopq", "a" * 15, "a" * 16, "a" * 17, "a" * 31, "a" * 32, "a" * 33, "a" * 63, "a" * 64, "a" * 65,
            "z" * 200, "internationalization", "internationalizations"]


def added_docs():
    return [SOT, SOT.upper(), "<|StartOfText|>", "a " + SOT.upper() + " b", "a" + SOT + "'s", EOT, EOT.upper(), "x" + EOT + "y", EOT + EOT, SOT + EOT, "it" + EOT + "'s",
            "a photo of a cat" + EOT, SOT + "A PHOTO" + EOT, "<|startoftext", "|>", DOTTED_I + SOT + DOTTED_I, "é" + EOT + "́x"]


def norm_docs():
    return ["École", "ÉCOLE", "Ǻ", "Å", "K", "ſ", DOTTED_I, DOTTED_I * 3, "İ", "x" + DOTTED_I + "y", "ǅ", "ß", "ẞ", "Σ", "ΑΣ",
            "ﬁ", "中文", "가", "가", "각", "́", "́a", "ạ́", "ạ́", "A" + "́" * 30, "\U0001f601\u200d\U0001f601",
            "٣٤", "½", "Ⅷ", "\U0001d7ce", "٠a١", "CAFÉ CAFÉ café", "ẛ̣", "क़", "ཱི", "Ḍ̇"]


def all_docs():
    """the vectors' documents: the whole batch has more than two workgroups of text and a count that is no multiple of 256"""
    docs = edge_docs() + run_docs() + last_byte_docs() + added_docs() + norm_docs()
    docs += ["A  photo of\tÉcole's " + DOTTED_I + " café!!", "Hello, y'all! How are you \U0001f601 ?", "a photo of a cat", "An oil painting of the MOUNTAINS at sunset, highly detailed"]
    docs += random_docs(300, seed=7)
    if len(docs) % 256 == 0:
        docs.append("pad")
    return docs


def prompts(n=96, seed=11):
    """short prompts, as CLIP batches are"""
    rng = random.Random(seed)
    words = [w for w in MERGE_WORDS if w.isalpha() and w.isascii()] + ["A", "Photo", "OF", "4k", "8K", "it's", "artist's", "don't"]
    return [" ".join(rng.choice(words) for _ in range(rng.randint(1, 110))) + rng.choice(["", ".", "!!", " ...", "?"]) for _ in range(n)]
