"""The seeded cross-layout differential's generator, as a pure function: make_case(name, seed) takes a tokenizer fixture and mixes, across its
components, what every layout's own suite runs only as shipped -- the post-processor is rewritten, one to six added tokens of random shape
are added, truncation / padding sections are drawn, the options of the components on the path are flipped, and the input is single
sequences, pairs, pre-tokenized words, pairs of those or a mixture, of random -- deliberately nasty -- Unicode.  Nothing here imports the
library or the wheel: tools/fuzz_live.py runs cases live against the wheel, tools/make_golden_fuzz.py records the wheel's answers for seeds
0..11 of every family (tests/golden/fuzz_layouts_vectors.json.gz), tests/test_fuzz_layouts.py pins the generator to those vectors by
digest and tests/test_fuzz_layouts_gpu.py holds the device to them.  found_cases() are the reduced cases of what the differential found."""
import hashlib
import json
import os
import random

from tests.helpers import GOLD, load_tokenizer_json, load_vectors

# the fixtures whose load dominates a case (50 k .. 128 k vocabularies): run them by name with tools/fuzz_live.py
HEAVY = ("gpt2_synth_50257", "gpt2_added_tokens", "gpt2_added_quirk", "gpt2_bench_added", "nfc_gpt2", "llama3_128k", "bert_wordpiece_30522")
# every other tokenizer fixture under tests/golden/ (a *_vectors file is no tokenizer, nor is what the loader made of them all,
# tools/make_golden_host_model.py)
FAMILIES = sorted(f[:-len(".json.gz")] for f in os.listdir(GOLD)
                  if f.endswith(".json.gz") and not f.endswith("_vectors.json.gz") and f[:-len(".json.gz")] not in HEAVY + ("host_model_outcomes",))
SEEDS = tuple(range(12))
MAX_DOCS, MAX_CHARS = 24, 120

ALPHA = [
    "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ", "      ", " \t\n\r", "0123456789", ".,;:!?'\"()[]{}-_/\\@#$%^&*+=<>|~`",
    "'s't're've'm'll'd'S'T'RE",
    "éèêëàâäôöùûüçñßÀÉÖÜÇÑ",
    "़゙्ְֹًّཱིུ̧̨̛̣〮〯̀́̂̃̈ͅ",
    "中文字符漢字日本語", "ひらがなカタカナ", "한국어글자각",
    "각히", "\U0001f600\U0001f389\U0001f44d\U0001f3fd\U0001f468‍\U0001f469‍\U0001f467\U0001f1eb\U0001f1f7",
    "      　​‍﻿­  ",
    "\x00\x01\x07\x1f\x7f�", "АБВгдежЯяΩωαβγ",
    "ﬁﬃǅǆİıſẞ", "ابتثجحخ שלום",
    "\U00010400\U0001d400\U0002f800\U000e0001\U0010ffff", "½¼²³№™©®", "İIıiΣσς",
]
ADDED_POOL = ["ing", "the", " a", "<x>", "[Y]", "é", "İ", "中", "##s", "ab ", " '", "１", "Ab", "AB", "\n", "a b",
              "<x", "x>", "<x><y>", "ab", "abc", "b", "bc", "e\u0301", "\u00c9", "  ", "\t", "a", "A", "<X>", "i\u0307", "ı", "ﬁ", "fi", "ǆ"]
CHAIN_TYPES = ("NFD", "Lowercase", "StripAccents")


def _text(rnd, maxlen):
    n = rnd.choice([0, 1, 2, 3, 5, 8, 13, 30, 60, maxlen])
    out = []
    while len(out) < n:
        a = rnd.choice(ALPHA if rnd.random() < 0.5 else ALPHA[:6])
        for _ in range(rnd.randint(1, 6)):
            out.append(rnd.choice(a))
    return "".join(out[:maxlen])


def _members(section, key):
    """the component itself, or the members of its Sequence"""
    if not section:
        return []
    return section.get(key, []) if section["type"] == "Sequence" else [section]


def _mix_components(rnd, d):
    """the options of the components on the path, at random"""
    nz, pt, mdl = d.get("normalizer"), d.get("pre_tokenizer"), d["model"]
    if nz and nz["type"] == "BertNormalizer" and rnd.random() < 0.5:
        nz.update(clean_text=rnd.random() < 0.7, handle_chinese_chars=rnd.random() < 0.7, strip_accents=rnd.choice([None, True, False]), lowercase=rnd.random() < 0.6)
    chain = _members(nz, "normalizers")
    if chain and all(m["type"] in CHAIN_TYPES for m in chain) and rnd.random() < 0.4:
        # a random in-order subset of an NFD / Lowercase / StripAccents chain (never none of them: the file's own spelling of "one" is kept)
        keep = [m for m in chain if rnd.random() < 0.6] or [rnd.choice(chain)]
        d["normalizer"] = keep[0] if len(keep) == 1 and rnd.random() < 0.5 else {"type": "Sequence", "normalizers": keep}
    if pt and pt["type"] == "ByteLevel" and rnd.random() < 0.5:
        pt.update(add_prefix_space=rnd.random() < 0.5, use_regex=rnd.random() < 0.8)
    if pt and pt["type"] in ("BertPreTokenizer", "Whitespace", "WhitespaceSplit") and rnd.random() < 0.3:
        d["pre_tokenizer"] = {"type": rnd.choice(["BertPreTokenizer", "Whitespace", "WhitespaceSplit"])}
    for m in _members(pt, "pretokenizers"):
        if m["type"] == "Metaspace" and rnd.random() < 0.25:
            m.pop("add_prefix_space", None)
            m["prepend_scheme"] = rnd.choice(["always", "first", "never"])
        if m["type"] == "Digits" and rnd.random() < 0.3:
            m["individual_digits"] = not m.get("individual_digits", False)
    if d.get("post_processor") and d["post_processor"]["type"] == "ByteLevel" and rnd.random() < 0.5:
        d["post_processor"].update(add_prefix_space=rnd.random() < 0.5, trim_offsets=rnd.random() < 0.7)
    if mdl["type"] == "WordPiece" and rnd.random() < 0.3:
        mdl["max_input_chars_per_word"] = rnd.choice([3, 6, 100])
    if mdl["type"] == "BPE" and rnd.random() < 0.1:               # (refused over whole "▁" pieces and with an end_of_word_suffix: rarely, for the 8-of-12 cap)
        mdl["ignore_merges"] = not mdl.get("ignore_merges", False)


def _mix_added_tokens(rnd, d):
    """a few added tokens of random shape (their ids follow the reference's rule whatever is written here)"""
    have = {a["content"] for a in d["added_tokens"]}
    # (a normalized token is refused at load behind the Precompiled and the "▁" normalizers, which match on the normalized text: rare there,
    # so that 8 of a family's 12 cases load)
    kinds = {m["type"] for m in _members(d.get("normalizer"), "normalizers")}
    p_normalized = 0.1 if kinds & {"Precompiled", "Prepend"} or ("Replace" in kinds and "NFC" not in kinds) else 0.5
    for c in rnd.sample(ADDED_POOL, rnd.randint(1, 6)):
        # (a content the file already holds, with OTHER properties, is where the 0.22.2 wheel and the reference tree part: the wheel
        # keeps the stale entry in its pattern lists -- both the old and the new token match --, the tree builds its tries from the
        # id -> token map, added_vocabulary.rs:379-399: last properties only, which is what the library does.  Found by seed 60602.)
        if c in have:
            continue
        d["added_tokens"].append({"id": 0, "content": c, "single_word": rnd.random() < 0.3, "lstrip": rnd.random() < 0.3, "rstrip": rnd.random() < 0.3,
                                  "normalized": rnd.random() < p_normalized, "special": rnd.random() < 0.4})


def _mix_post_processor(rnd, d):
    r = rnd.random()
    # (a trimming post-processor is refused over a vocabulary that is not byte-level and has whitespace-edged entries, as the "▁" files' are:
    # drawn half as often where no ByteLevel pre-tokenizer stands, for the 8-of-12 cap)
    p_trim = 1.0 if any(m["type"] == "ByteLevel" for m in _members(d.get("pre_tokenizer"), "pretokenizers")) else 0.5
    S = lambda i, t=0: {"SpecialToken": {"id": i, "type_id": t}}
    Q = lambda i, t=0: {"Sequence": {"id": i, "type_id": t}}
    sp = {"<a>": {"id": "<a>", "ids": [1], "tokens": ["<a>"]}, "<b>": {"id": "<b>", "ids": [2, 1], "tokens": ["<b>", "<a>"]}}
    if r < 0.1:
        d["post_processor"] = None
    elif r < 0.2:
        # (with both of Roberta's flags the tree and the wheel read either spelling as a RobertaProcessing: processors/mod.rs, untagged)
        d["post_processor"] = {"type": rnd.choice(["BertProcessing", "RobertaProcessing"]), "sep": ["<s>", 1], "cls": ["<c>", 2], "trim_offsets": rnd.random() < 0.5 * p_trim, "add_prefix_space": rnd.random() < 0.5}
    elif r < 0.4:
        t = [rnd.choice([0, 0, 1, 2]) for _ in range(8)]
        d["post_processor"] = {"type": "TemplateProcessing", "special_tokens": sp,
                               "single": rnd.choice([[S("<a>", t[0]), Q("A", t[1])], [Q("A", t[1]), S("<b>", t[2])], [S("<b>", t[0]), Q("A", t[1]), S("<a>", t[2])], [Q("A", t[1])]]),
                               "pair": rnd.choice([[S("<a>", t[3]), Q("A", t[4]), S("<b>", t[5]), Q("B", t[6]), S("<a>", t[7])], [Q("B", t[6]), Q("A", t[4])], [Q("A", t[4]), S("<b>", t[5]), Q("B", t[6])]])}
    elif r < 0.46:
        d["post_processor"] = {"type": "ByteLevel", "add_prefix_space": rnd.random() < 0.5, "trim_offsets": rnd.random() < 0.7 * p_trim, "use_regex": True}


def digest(case) -> str:
    """SHA-256 over everything a case hands to the two libraries: a drift of the generator is a failure, not another test"""
    blob = json.dumps([case["json"], case["inputs"], case["mode"], case["add_special_tokens"], case["encode_special_tokens"], case["is_pretokenized"]],
                      ensure_ascii=True, sort_keys=True)
    return hashlib.sha256(blob.encode("ascii")).hexdigest()


def make_case(name, seed, heavy_truncation=False, max_docs=MAX_DOCS):
    """case `seed` of fixture `name`: {"name", "seed", "json", "inputs", "mode", "add_special_tokens", "encode_special_tokens", "is_pretokenized"}.
    Deterministic: everything is drawn from random.Random(f"{name}:{seed}").  heavy_truncation: mostly truncated batches, short windows,
    wider strides (tools/fuzz_live.py with FUZZ_TRUNCATION=1; the recorded vectors are drawn without)."""
    rnd = random.Random(f"{name}:{seed}")
    d = json.loads(load_tokenizer_json(name))
    heavy = heavy_truncation
    if rnd.random() < (0.9 if heavy else 0.3):
        d["truncation"] = {"direction": rnd.choice(["Right", "Left"]), "max_length": rnd.choice([2, 3, 4, 5, 7, 9, 12] if heavy else [4, 7, 16, 40]),
                           "strategy": rnd.choice(["LongestFirst", "OnlyFirst", "OnlySecond"]), "stride": rnd.choice([0, 1, 2, 3] if heavy else [0, 1])}
    if rnd.random() < 0.3:
        d["padding"] = {"strategy": rnd.choice(["BatchLongest", {"Fixed": 24}]), "direction": rnd.choice(["Right", "Left"]),
                        "pad_to_multiple_of": rnd.choice([None, 8]), "pad_id": 0, "pad_type_id": 1, "pad_token": "[PAD]"}
    _mix_components(rnd, d)
    if rnd.random() < 0.35:
        _mix_added_tokens(rnd, d)
    _mix_post_processor(rnd, d)
    mode = rnd.choice(["single", "single", "pair", "words", "wordpairs", "mixed", "mixedwords"])
    special = rnd.random() < 0.5
    docs = [_text(rnd, MAX_CHARS) for _ in range(rnd.randint(1, max_docs))]
    if rnd.random() < 0.3:                       # text made of the added tokens, their fragments and whitespace
        frag = [a["content"] for a in d["added_tokens"]] + [a["content"][:-1] for a in d["added_tokens"] if len(a["content"]) > 1] + \
               [a["content"].upper() for a in d["added_tokens"]] + [" ", "  ", "\t", "\n", "a", "b", "x", ".", "'", "é", "İ"]
        docs = ["".join(rnd.choice(frag) for _ in range(rnd.randint(0, 16)))[:MAX_CHARS] for _ in range(rnd.randint(1, max_docs))]
    if mode == "single":
        inputs = docs
    elif mode == "pair":
        inputs = [[docs[i], docs[-1 - i]] for i in range((len(docs) + 1) // 2)]
    elif mode == "words":
        inputs = [x.split(" ") if rnd.random() < 0.8 else [] for x in docs]
    elif mode == "mixed":
        inputs = [docs[i] if rnd.random() < 0.5 else [docs[i], docs[-1 - i]] for i in range(len(docs))]
    elif mode == "mixedwords":
        inputs = [docs[i].split(" ") if rnd.random() < 0.5 else [docs[i].split(" "), docs[-1 - i].split(" ")] for i in range(len(docs))]
    else:
        inputs = [[docs[i].split(" "), docs[-1 - i].split(" ")] for i in range((len(docs) + 1) // 2)]
    return {"name": name, "seed": seed, "json": json.dumps(d, ensure_ascii=False), "inputs": inputs, "mode": mode, "add_special_tokens": special,
            "encode_special_tokens": rnd.random() < 0.15, "is_pretokenized": mode in ("words", "wordpairs", "mixedwords")}


def call_inputs(case):
    """the inputs as encode_batch takes them: a pair is a tuple (JSON, and so the cases, know lists only)"""
    pre = case["is_pretokenized"]

    def one(x):
        is_pair = isinstance(x, list) and len(x) == 2 and isinstance(x[0], list) if pre else isinstance(x, list)
        return tuple(x) if is_pair else x
    return [one(x) for x in case["inputs"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# What the differential found (seeds 101-103, 201-203 of tools/fuzz_live.py over the newer layouts), each reduced to the tokenizer
# edit and the smallest inputs that differed from the wheel.
# ---------------------------------------------------------------------------------------------------------------------------------
def _edited(name, *, post_processor="keep", added=(), padding=None):
    d = json.loads(load_tokenizer_json(name))
    if post_processor != "keep":
        d["post_processor"] = post_processor
    for content, props in added:
        a = {"id": 0, "content": content, "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False}
        a.update(props)
        d["added_tokens"].append(a)
    if padding:
        d["padding"] = padding
    return json.dumps(d, ensure_ascii=False)


def _found(name, js, inputs, mode="single", special=False, esp=False):
    return {"name": name, "seed": None, "json": js, "inputs": inputs, "mode": mode, "add_special_tokens": special, "encode_special_tokens": esp,
            "is_pretokenized": mode in ("words", "wordpairs", "mixedwords")}


def found_cases():
    """finding -> its cases.  The names say what the device must do."""
    trimming = lambda ty, aps=True: {"type": ty, "sep": ["<s>", 1], "cls": ["<c>", 2], "trim_offsets": True, "add_prefix_space": aps}
    ws_docs = ["\r", "dT''S\t\t\t", "\t\tab\t\t", "a \r\n b", "  x　 ", "中\t", "\t", "x \x0b y", "", "ab"]
    out = {}
    # F1 (seeds 101, 103, 201, 202): the token of a Unigram unknown run is the run's own text, so a trimming post-processor takes the
    # whitespace at its edges off its offsets ("\r" -> (0, 0), "dT''S\t\t\t" -> ends at 5)
    out["trimming_post_processor_trims_a_unigram_unknown_run_over_whitespace"] = [
        _found(name, _edited(name, post_processor=trimming(ty, aps)), docs, mode, special)
        for name in ("precompiled_ms", "unigram_adv") for ty in ("RobertaProcessing", "BertProcessing") for aps in (True, False)
        for docs, mode, special in ((ws_docs, "single", False), ([x.split(" ") for x in ws_docs], "words", True))]
    # F2 (seed 102): behind CLIP's Replace(\s+ -> " ") a normalized added token "  " is the pattern " ", which is also what "\t" becomes:
    # the word is that token, not nothing.  With it: a " " inside a pattern is a whole run; the one " " a run becomes stands where the
    # run's last char stood (lstrip swallows that one char; a match that opens with it starts there); single_word looks in front of the run
    two_spaces = [("  ", {"single_word": True, "rstrip": True})]
    runs = [(" x", {}), ("a b", {}), ("q", {"lstrip": True, "rstrip": True})]
    first_wins = [(" ", {"lstrip": True}), ("\t", {})]
    single_docs = ["\t", ". .", ".\t\t.", "a\t.", "\t\ta", " . ", "  ", "", "a<İ  'x", "é́  .", " x"]
    out["whitespace_of_a_normalized_added_token_is_one_space_behind_clips_replace"] = [
        _found("clip_bpe", _edited("clip_bpe", added=two_spaces), [["\t"], ["a", "\t", "b"], ["", " "], ["\t\t", "x"]], "words", esp=True),
        _found("clip_bpe", _edited("clip_bpe", added=two_spaces), single_docs),
        _found("clip_bpe", _edited("clip_bpe", added=runs), [".\t\n x", "\t\n x", "a \t b", "a b", ". \t q\n\n .", "a  \tb a b a 　b", " x", "x x", ".q", "  q", "a \t"]),
        _found("clip_bpe_plain", _edited("clip_bpe_plain", added=first_wins), single_docs),
        _found("clip_bpe", _edited("clip_bpe", added=first_wins, post_processor=None), [[d, d[::-1]] for d in single_docs], "pair", True),
    ]
    # F3 (seed 203): the same token missing from ONE member made every member of a BatchLongest batch one pad short
    pad = {"strategy": "BatchLongest", "direction": "Right", "pad_to_multiple_of": 8, "pad_id": 0, "pad_type_id": 1, "pad_token": "[PAD]"}
    S = lambda i, t=0: {"SpecialToken": {"id": i, "type_id": t}}
    Q = lambda i, t=0: {"Sequence": {"id": i, "type_id": t}}
    template = {"type": "TemplateProcessing", "special_tokens": {"<b>": {"id": "<b>", "ids": [2, 1], "tokens": ["<b>", "<a>"]}},
                "single": [Q("A"), S("<b>")], "pair": [Q("B"), Q("A", 2)]}
    added = [("[Y]", {"special": True}), ("x>", {"normalized": False}), ("a b", {}), ("abc", {"single_word": True, "lstrip": True, "rstrip": True, "normalized": False}),
             ("  ", {"lstrip": True}), ("AB", {"single_word": True, "lstrip": True, "normalized": False, "special": True})]
    out["padded_batch_of_word_pairs_counts_the_whitespace_token_of_every_member"] = [
        _found("clip_bpe_plain", _edited("clip_bpe_plain", post_processor=template, added=added, padding=pad),
               [[["", "", "xx>", ""], ["é.x>é", "", "a", "AB"]], [["[Y]İ<|startoftext|>\tbaab<|endoftext|A", "Babc[Y]"], ["", "Aİ"]]], "wordpairs"),
    ]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# What is recorded of an answer, and how (the wheel's Encoding and the library's carry the same attributes)
# ---------------------------------------------------------------------------------------------------------------------------------
_VECTORS = {}


def vectors():
    """tests/golden/fuzz_layouts_vectors.json.gz (tools/make_golden_fuzz.py), read once"""
    if not _VECTORS:
        _VECTORS.update(load_vectors("fuzz_layouts"))
    return _VECTORS


FIELDS = ("ids", "type_ids", "attention_mask", "special_tokens_mask", "offsets", "word_ids", "sequence_ids")
REFUSAL_CHARS = 60


def fields(e):
    """the seven arrays of one encoding, as JSON holds them: offsets flat, None as -1"""
    flat = [int(x) for o in e.offsets for x in o]
    opt = lambda xs: [-1 if x is None else int(x) for x in xs]
    return [[int(x) for x in e.ids], [int(x) for x in e.type_ids], [int(x) for x in e.attention_mask], [int(x) for x in e.special_tokens_mask],
            flat, opt(e.word_ids), opt(e.sequence_ids)]


def deep(e):
    """an encoding and each of its overflowing ones"""
    return [fields(e)] + [fields(o) for o in e.overflowing]


def decode_sequences(case, encoded_ids):
    """what decode_batch is asked: the encoded ids, and four of them shuffled (sequences no encoder would produce)"""
    rnd = random.Random(f"{case['name']}:{case['seed']}:decode")
    return [list(x) for x in encoded_ids] + [rnd.sample(list(x), len(x)) for x in encoded_ids[:4]]
