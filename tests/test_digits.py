"""Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family (PT_DIGITS_GPT2), the CPU side: which tokenizer.json shapes load and
which are refused (by message); the UC_RUST_N flag of the class table against the reference wheel's Digits, scalar by scalar; and the
host+device core tokenizers_amd/csrc/pretok_digits_core.hpp -- what every lane of k_pretok_digits executes, through
tests/harness/digits_harness.cpp, built with g++ -- against the wheel's own Sequence."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from oracle import synth
from tests import digits_cases as dc
from tests import word_edge_totals as wt
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "digits_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_digits_harness.so")
IND, CON = dc.NAMES
UC_ONIG_N, UC_RUST_N = 2, 128


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("pretok_digits_core.hpp", "pretok_gpt2_core.hpp", "unicode_numeric_ranges.inc", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.dgh_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.dgh_run.restype = C.c_int
    lib.dgh_classes.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    lib.dgh_classes.restype = C.c_int
    return lib


def _file(name=IND, **over):
    d = json.loads(load_tokenizer_json(name))
    d.update(over)
    return json.dumps(d, ensure_ascii=False)


DIGITS = {"type": "Digits", "individual_digits": True}
BYTELEVEL = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}


def _seq(*members, **over):
    return _file(pre_tokenizer={"type": "Sequence", "pretokenizers": list(members)}, **over)


# ---- 1. load and refuse ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.NAMES)
def test_the_fixture_loads_as_the_new_kind(name):
    tok = ta.Tokenizer.from_str(load_tokenizer_json(name), device=-1)
    assert tok.info["pre_tokenizer"] == 9 and tok.info["normalizer"] == 0 and tok.info["model"] == 1


def test_normalizers_and_trim_offsets_that_load():
    for norm, kind in ((None, 0), ({"type": "Sequence", "normalizers": []}, 0), ({"type": "NFC"}, 3), ({"type": "Sequence", "normalizers": [{"type": "NFC"}]}, 3)):
        info = ta.Tokenizer.from_str(_file(normalizer=norm), device=-1).info
        assert (info["pre_tokenizer"], info["normalizer"]) == (9, kind), norm
    assert ta.Tokenizer.from_str(_seq(DIGITS, dict(BYTELEVEL, trim_offsets=False)), device=-1).info["pre_tokenizer"] == 9
    assert ta.Tokenizer.from_str(_seq({"type": "Digits"}, BYTELEVEL), device=-1).info["pre_tokenizer"] == 9      # (individual_digits defaults to false)


WORDPIECE = {"type": "WordPiece", "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100, "vocab": {"[UNK]": 0, "a": 1}}
REFUSED = [
    (_seq(DIGITS, dict(BYTELEVEL, add_prefix_space=True)), r"Sequence\[Digits, ByteLevel\(add_prefix_space=true\)\]"),
    (_seq(DIGITS, dict(BYTELEVEL, use_regex=False)), r"Sequence\[Digits, ByteLevel\(use_regex=false\)\]"),
    (_seq(BYTELEVEL, DIGITS), "Digits behind ByteLevel reads the byte-level alphabet.*Falcon"),
    (_seq({"type": "Punctuation", "behavior": "Contiguous"}, dict(BYTELEVEL, use_regex=False), dict(DIGITS, individual_digits=False),
          {"type": "Split", "pattern": {"Regex": "[0-9][0-9][0-9]"}, "behavior": "Isolated", "invert": False}), "Digits behind ByteLevel.*Falcon's"),
    (_seq({"type": "Punctuation", "behavior": "Contiguous"}, DIGITS, BYTELEVEL), "Digits in a chain of 3 pre-tokenizers.*Falcon's"),
    (_seq(DIGITS, DIGITS, BYTELEVEL), "Digits in a chain of 3"),
    (_seq({"type": "Whitespace"}, DIGITS), "Digits in a chain of 2"),
    (_seq(DIGITS), "Digits in a chain of 1"),
    (_seq(DIGITS, {"type": "Whitespace"}), r"Sequence\[Digits, Whitespace\]"),
    (_file(pre_tokenizer=DIGITS), "Digits alone is outside the hot path"),
    (_file(model=WORDPIECE, added_tokens=[], post_processor=None, decoder=None), r"Sequence\[Digits, ByteLevel\] in front of a WordPiece model"),
    (_file(model={"type": "WordLevel", "vocab": {"[UNK]": 0, "a": 1}, "unk_token": "[UNK]"}, added_tokens=[], post_processor=None, decoder=None),
     r"Sequence\[Digits, ByteLevel\] in front of a WordLevel model"),
    (_file(model={"type": "Unigram", "unk_id": 0, "vocab": [["<unk>", 0.0], ["a", -1.0]], "byte_fallback": False}, added_tokens=[], post_processor=None, decoder=None),
     r"Sequence\[Digits, ByteLevel\] in front of a Unigram model"),
    (_file(normalizer={"type": "NFKC"}), "normalizer: type 'NFKC' is outside the hot path"),
    (_file(normalizer={"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None, "lowercase": False}),
     r"Sequence\[Digits, ByteLevel\] behind a normalizer other than NFC"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_near_misses_are_refused_by_reason(k):
    js, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        ta.Tokenizer.from_str(js, device=-1)


# ---- 2. classes ------------------------------------------------------------------------------------------------------------------------

def _flags(lib, name):
    jb = load_tokenizer_json(name).encode("utf-8")
    flags = np.zeros(0x110000, dtype=np.uint8)
    assert lib.dgh_classes(jb, len(jb), flags.ctypes.data) == 0
    return flags


def test_numeric_flag_equals_the_wheels_digits(harness, ref_tokenizers):
    """for every scalar value: UC_RUST_N of the table the loader builds == Digits(individual_digits=True) makes the char a piece of its own"""
    flags = _flags(harness, IND)
    digits = ref_tokenizers.pre_tokenizers.Digits(individual_digits=True)
    cps = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]
    member = np.zeros(0x110000, dtype=bool)
    for k in range(0, len(cps), 0x8000):
        part = cps[k:k + 0x8000]
        for _, (a, b) in digits.pre_tokenize_str("".join("a" + chr(cp) for cp in part) + "a"):
            if b - a == 1 and a % 2 == 1:
                member[part[a // 2]] = True
    bad = np.nonzero(member != ((flags & UC_RUST_N) != 0))[0]
    assert len(bad) == 0, [hex(int(x)) for x in bad[:8]]
    assert int(member.sum()) == 1924
    # the two numeric classes: the regex engine's \p{N} is inside char::is_numeric, thirteen chars short
    onig = (flags & UC_ONIG_N) != 0
    assert not (onig & ~member).any()
    assert [int(x) for x in np.nonzero(member & ~onig)[0]] == list(range(0x11DE0, 0x11DEA)) + list(range(0x16FF4, 0x16FF7))
    # ASCII: what the kernel's byte table says without a table load
    assert [v for v in range(128) if member[v]] == list(range(0x30, 0x3A))


def test_the_flag_touches_no_other_handle_and_no_other_bit(harness):
    """the table of every other kind is the parent's: the flag is ORed in for PT_DIGITS_GPT2 alone, and there it changes bit 7 only"""
    base, ours = _flags(harness, "split_qwen2"), _flags(harness, CON)
    assert not (base & UC_RUST_N).any()
    assert np.array_equal(base, ours & ~np.uint8(UC_RUST_N))


# ---- 3. the core against the wheel's Sequence ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wheel(ref_tokenizers):
    return {name: ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(name)).pre_tokenizer for name in dc.NAMES}


def _pack(docs):
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy(), off


def _expected(pretok, docs, off):
    """-> (piece starts, lead bytes), one byte per text byte"""
    exp, lead = np.zeros(int(off[-1]), dtype=np.uint8), np.zeros(int(off[-1]), dtype=np.uint8)
    for d, text in enumerate(docs):
        m = np.cumsum([0] + [len(c.encode("utf-8")) for c in text])
        lead[off[d] + m[:-1]] = 1
        for _, (a, _b) in pretok.pre_tokenize_str(text):
            exp[off[d] + m[a]] = 1
    return exp, lead


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n]


def _run_core(lib, name, buf, off):
    jb = load_tokenizer_json(name).encode("utf-8")
    n, nd = int(off[-1]), len(off) - 1
    st, ld = np.zeros((n >> 6) + 1, dtype=np.uint64), np.zeros((n >> 6) + 1, dtype=np.uint64)
    assert lib.dgh_run(jb, len(jb), buf.ctypes.data, n, off.ctypes.data, nd, st.ctypes.data, ld.ctypes.data) == 0
    assert not _bits(st, 64 * len(st))[n:].any() and not _bits(ld, 64 * len(ld))[n:].any(), "bits behind the text's end"
    return _bits(st, n), _bits(ld, n)


def _first_bad(bad, off, docs, got, exp):
    g = int(bad[0])
    d = int(np.searchsorted(off, g, side="right") - 1)
    return f"{len(bad)} wrong bytes; first at doc {d} byte {g - off[d]}: {docs[d][:80]!r} got={got[g]} wheel={exp[g]}"


def _hold(name, got, lead, exp, exp_lead, off, docs):
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, f"{name}: " + _first_bad(bad, off, docs, got, exp)
    bad = np.nonzero(lead != exp_lead)[0]
    assert len(bad) == 0, f"{name}, lead mask: " + _first_bad(bad, off, docs, lead, exp_lead)


def _check(lib, wheel, docs, names=dc.NAMES):
    buf, off = _pack(docs)
    for name in names:
        got, lead = _run_core(lib, name, buf, off)
        exp, exp_lead = _expected(wheel[name], docs, off)
        _hold(name, got, lead, exp, exp_lead, off, docs)


def test_table_of_the_issue(harness, wheel):
    for text, individual, contiguous in dc.TABLE:
        for name, pieces in ((IND, individual), (CON, contiguous)):
            if pieces is not None:
                assert [p for p, _ in wheel[name].pre_tokenize_str(text)] == pieces, (name, text)
    text = dc.TABLE[-1][0]
    got = [text[a:b] for _, (a, b) in wheel[IND].pre_tokenize_str(text)]
    assert got == dc.TABLE_WIDE_INDIVIDUAL
    # the two numeric classes: one piece, two pre-tokens
    assert [o for _, o in wheel[CON].pre_tokenize_str("1\U00011DE02")] == [(0, 1), (1, 2), (2, 3)]
    _check(harness, wheel, [t for t, _, _ in dc.TABLE])


def test_edge_documents_alone_and_in_batches(harness, wheel):
    for d in dc.edge_docs():                              # alone: at byte 0 of its batch
        if len(d) < 2000:
            _check(harness, wheel, [d])
    long_docs = [d for d in dc.edge_docs() if len(d) >= 2000]
    assert len(long_docs) >= 30
    for k in range(0, len(long_docs), 3):                 # (the 16 KB ones: alone for a third of them, every one first in a batch of three)
        _check(harness, wheel, [long_docs[k]])
        _check(harness, wheel, long_docs[k:k + 3])
    for b in dc.batches():
        _check(harness, wheel, b)
    _check(harness, wheel, [d for d in dc.edge_docs() if len(d) < 2000])


@pytest.mark.parametrize("total", wt.TOTALS)
def test_total_lengths_at_the_workgroup_edge(total, harness, wheel):
    """the text's last word, the position n_bytes and the edge of a workgroup together: one document and two"""
    for docs in wt.batches(total):
        _check(harness, wheel, docs)


def test_exhaustive_short_strings_at_every_word_offset(harness, wheel):
    """every string of length <= 4 over the 9-symbol alphabet, each a document of its own, the batch behind a filler document of 0..63
    bytes: each string meets every offset of a 64-byte mask word.  The wheel is asked once: its answer does not depend on the filler."""
    strings = ["".join(t) for n in range(1, 5) for t in itertools.product(dc.ALPHABET, repeat=n)]
    assert len(strings) == sum(9 ** n for n in range(1, 5))
    buf0, off0 = _pack(strings)
    for name in dc.NAMES:
        exp0, lead0 = _expected(wheel[name], strings, off0)
        for shift in range(64):
            buf = np.concatenate([np.full(shift, ord("x"), dtype=np.uint8), buf0])
            off = np.concatenate([[0], off0 + shift]).astype(np.int64)
            head = np.zeros(shift, dtype=np.uint8)
            head[:1] = 1
            got, lead = _run_core(harness, name, buf, off)
            _hold(name, got, lead, np.concatenate([head, exp0]), np.concatenate([np.ones(shift, dtype=np.uint8), lead0]), off, ["x" * shift] + strings)


def test_exhaustive_short_strings_in_one_document(harness, wheel):
    """the same strings without document edges between them: joined by a letter into one document, so every piece edge is Digits' own"""
    strings = ["".join(t) for n in range(1, 5) for t in itertools.product(dc.ALPHABET, repeat=n)]
    for sep in ("b", " ", "2"):
        _check(harness, wheel, [sep.join(strings), "x" * 37 + sep.join(reversed(strings))])


def test_seeded_random_strings(harness, wheel):
    for seed in range(3):
        _check(harness, wheel, dc.random_strings(3000, seed=400 + seed))
        _check(harness, wheel, dc.random_strings(3000, seed=410 + seed, alphabet=dc.WIDE))
    _check(harness, wheel, dc.random_strings(20000, seed=420, lo=0, hi=24, alphabet=dc.WIDE))
    # long texts in ONE document each: several workgroups of 16384 bytes
    _check(harness, wheel, ["".join(dc.random_strings(400, seed=430, alphabet=dc.WIDE)), dc.big_doc(), dc.mixed_text(5000, seed=5)])
    _check(harness, wheel, synth.gen_lines(2000, text_seed=3) + synth.stress_lines(seed=4, n=500))
