"""The CLIP layout (Sequence[NFC, Replace(\\s+), Lowercase] + Split(the CLIP pattern, Removed, inverted) + ByteLevel + byte-level BPE with
end_of_word_suffix), the CPU side: which tokenizer.json shapes load and which are refused (by message); the pre-tokenizer core
tokenizers_amd/csrc/pretok_clip_core.hpp -- what every lane of k_pretok_clip executes, through tests/harness/clip_harness.cpp, built with
g++ -- against the wheel's own pre_tokenize_str; the NFC_LOWER mode of csrc/nfc_core.hpp against normalize_str of the wheel's chain; and the
whole device path under the SIMT emulation against the wheel's vectors."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import clip_cases as cc
from tests import word_edge_totals as wt
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "clip_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_clip_harness.so")
NAME = cc.NAMES[0]


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("pretok_clip_core.hpp", "pretok_gpt2_core.hpp", "nfc_core.hpp", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.clh_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.clh_run.restype = C.c_int
    lib.clh_normalize.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    lib.clh_normalize.restype = C.c_int64
    return lib


def _seq_norm(*members):
    return {"type": "Sequence", "normalizers": list(members)}


def _seq_pre(*members):
    return {"type": "Sequence", "pretokenizers": list(members)}


def _load(js):
    return ta.Tokenizer.from_str(js, device=-1)


# ---- 1. load and refuse ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.NAMES)
def test_the_fixture_loads_with_the_new_kinds(name):
    js = load_tokenizer_json(name)
    assert js == cc.file_of(normalized_sot=name == NAME)                       # (the committed file is the one tests/clip_cases.py builds)
    info = _load(js).info
    assert info["pre_tokenizer"] == 10 and info["normalizer"] == 7 and info["model"] == 1 and info["n_added_tokens"] == 2


def test_the_four_accepted_spellings_load():
    for norm in (_seq_norm(cc.NFC, cc.REPLACE, cc.LOWER), _seq_norm(cc.NFC, cc.LOWER)):
        for use_regex in (True, False):
            info = _load(cc.file_of(normalizer=norm, pre_tokenizer=_seq_pre(cc.SPLIT, dict(cc.BYTELEVEL, use_regex=use_regex)))).info
            assert (info["pre_tokenizer"], info["normalizer"]) == (10, 7), (norm, use_regex)
    assert _load(cc.file_of(pre_tokenizer=_seq_pre(cc.SPLIT, dict(cc.BYTELEVEL, trim_offsets=False)))).info["pre_tokenizer"] == 10


def _no_normalizer(**kw):
    d = json.loads(cc.file_of(**kw))
    d["normalizer"] = None
    return json.dumps(d, ensure_ascii=False)


def _vocab_without(entry):
    vocab = dict(json.loads(cc.file_of())["model"]["vocab"])
    del vocab[entry]
    return vocab


QWEN2 = "(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\\r\\n\\p{L}\\p{N}]?\\p{L}+|\\p{N}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+"
NFC_LONGER = "normalizer: NFC inside a longer Sequence is outside the hot path"
REFUSED = [
    # another pattern
    (cc.file_of(pre_tokenizer=_seq_pre(dict(cc.SPLIT, pattern={"Regex": cc.PATTERN + "|x"}), cc.BYTELEVEL)), NFC_LONGER + ".*this file's pre-tokenizer is another one"),
    (_no_normalizer(pre_tokenizer=_seq_pre(dict(cc.SPLIT, pattern={"Regex": cc.PATTERN.replace("[\\p{N}]", "\\p{N}")}), cc.BYTELEVEL)),
     "Split with behavior 'Removed' inverted \\(only Isolated is on the path; Removed, inverted, with the CLIP pattern alone"),
    # another behaviour or invert
    (cc.file_of(pre_tokenizer=_seq_pre(dict(cc.SPLIT, behavior="Isolated"), cc.BYTELEVEL)), "the CLIP Split pattern with behavior 'Isolated' inverted \\(only Removed, inverted"),
    (cc.file_of(pre_tokenizer=_seq_pre(dict(cc.SPLIT, invert=False), cc.BYTELEVEL)), "the CLIP Split pattern with behavior 'Removed', not inverted"),
    # add_prefix_space
    (cc.file_of(pre_tokenizer=_seq_pre(cc.SPLIT, dict(cc.BYTELEVEL, add_prefix_space=True))), r"Sequence\[Split\(the CLIP pattern\), ByteLevel\(add_prefix_space=true\)\]"),
    # the chain in another order, with another member, with another Replace
    (cc.file_of(normalizer=_seq_norm(cc.LOWER, cc.NFC)), NFC_LONGER + ".*other members, or these in another order"),
    (cc.file_of(normalizer=_seq_norm(cc.NFC, cc.LOWER, cc.REPLACE)), NFC_LONGER + ".*other members, or these in another order"),
    (cc.file_of(normalizer=_seq_norm(cc.NFC, cc.REPLACE, cc.LOWER, {"type": "StripAccents"})), NFC_LONGER + ".*other members, or these in another order"),
    (cc.file_of(normalizer=_seq_norm(cc.NFC, dict(cc.REPLACE, pattern={"Regex": " {2,}"}), cc.LOWER)), NFC_LONGER + ".*this Sequence's Replace is another one"),
    (cc.file_of(normalizer=_seq_norm(cc.NFC, dict(cc.REPLACE, content="_"), cc.LOWER)), NFC_LONGER + ".*this Sequence's Replace is another one"),
    (cc.file_of(normalizer=_seq_norm(cc.NFC, dict(cc.REPLACE, pattern={"String": " "}), cc.LOWER)), NFC_LONGER + ".*this Sequence's Replace is another one"),
    # the pre-tokenizer behind another normalizer
    (cc.file_of(normalizer=cc.NFC), "the CLIP Split is only on the path behind the normalizer"),
    (cc.file_of(normalizer=_seq_norm()), "the CLIP Split is only on the path behind the normalizer"),
    (cc.file_of(normalizer=cc.LOWER), "normalizer: type 'Lowercase' is outside the hot path in front of pre_tokenizer 'Sequence'"),
    # the chain in front of any other pre-tokenizer
    (cc.file_of(pre_tokenizer=cc.BYTELEVEL), NFC_LONGER + ".*this file's pre-tokenizer is another one"),
    (cc.file_of(pre_tokenizer=_seq_pre(dict(cc.SPLIT, pattern={"Regex": QWEN2}, behavior="Isolated", invert=False), dict(cc.BYTELEVEL, use_regex=False))),
     NFC_LONGER + ".*this file's pre-tokenizer is another one"),
    (cc.file_of(pre_tokenizer={"type": "Whitespace"}), NFC_LONGER),
    (cc.file_of(pre_tokenizer=_seq_pre(cc.SPLIT, {"type": "Whitespace"})), "this Sequence is outside the hot path"),
    # the model: a suffix on any other byte-level layout, a prefix, no suffix, what stays refused with one, the 512 entries
    (_no_normalizer(), "the CLIP Split is only on the path behind the normalizer"),
    (_no_normalizer(pre_tokenizer=cc.BYTELEVEL), "byte-level BPE with continuing_subword_prefix / end_of_word_suffix"),
    (cc.file_of(normalizer=cc.NFC, pre_tokenizer=dict(cc.BYTELEVEL, use_regex=False)), "byte-level BPE with continuing_subword_prefix / end_of_word_suffix"),
    (cc.file_of(model={"continuing_subword_prefix": "##"}), "byte-level BPE with continuing_subword_prefix / end_of_word_suffix"),
    (cc.file_of(model={"end_of_word_suffix": ""}), "the CLIP Split \\+ ByteLevel in front of a BPE without end_of_word_suffix"),
    (cc.file_of(model={"end_of_word_suffix": None}), "the CLIP Split \\+ ByteLevel in front of a BPE without end_of_word_suffix"),
    (cc.file_of(model={"end_of_word_suffix": "<" + "/" * 30 + ">"}), "end_of_word_suffix longer than 31 bytes"),
    (cc.file_of(model={"dropout": 0.1}), "BPE dropout"),
    (cc.file_of(model={"byte_fallback": True}), "byte-level BPE with byte_fallback"),
    (cc.file_of(model={"ignore_merges": True}), "byte-level BPE with end_of_word_suffix and ignore_merges"),
    (cc.file_of(model={"vocab": _vocab_without("q</w>")}), "the vocab lacks 'q</w>'"),
    (cc.file_of(model={"vocab": _vocab_without(cc.to_alphabet(" ") + "</w>")}), "the vocab lacks 'Ġ</w>'"),
    (cc.file_of(model={"vocab": _vocab_without("q")}), "byte-level BPE vocab lacks a byte symbol.*: 'q'"),
    (cc.file_of(model={"type": "WordLevel", "vocab": {"a": 0}, "unk_token": "a"}), r"the CLIP Split \+ ByteLevel in front of a WordLevel model"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_near_misses_are_refused_by_reason(k):
    js, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        _load(js)


def test_pinned_neighbours_keep_their_messages():
    """what the existing tests pin as refused, asked once more next to the new layout"""
    nl = _seq_norm(cc.NFC, cc.LOWER)
    for name in ("split_qwen2", "ds3_chain"):
        d = json.loads(load_tokenizer_json(name))
        d["normalizer"] = nl
        with pytest.raises(ta.UnsupportedError, match="NFC inside a longer Sequence"):
            _load(json.dumps(d))
    d = json.loads(load_tokenizer_json("split_qwen2"))
    d["pre_tokenizer"]["pretokenizers"][0]["behavior"] = "Removed"
    with pytest.raises(ta.UnsupportedError, match=r"Split with behavior 'Removed' \(only Isolated is on the path\)"):
        _load(json.dumps(d))
    d = json.loads(load_tokenizer_json("gpt2_synth_50257"))
    d["normalizer"] = cc.LOWER
    with pytest.raises(ta.UnsupportedError, match="normalizer: type 'Lowercase' is outside the hot path in front of pre_tokenizer 'ByteLevel'"):
        _load(json.dumps(d))
    d["normalizer"] = None
    d["model"]["end_of_word_suffix"] = "</w>"
    with pytest.raises(ta.UnsupportedError, match="byte-level BPE with continuing_subword_prefix / end_of_word_suffix"):
        _load(json.dumps(d))


# ---- 2. the pre-tokenizer core against the wheel's pre_tokenize_str -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def wheel(ref_tokenizers):
    return ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(NAME))


def _pack(docs):
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy(), off


def _expected(pretok, docs, off):
    """-> (pre-token starts, ends, lead bytes): one byte per text byte, and one more for the position behind the text"""
    n = int(off[-1])
    st, en, lead = np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint8)
    for d, text in enumerate(docs):
        m = np.cumsum([0] + [len(c.encode("utf-8")) for c in text])
        lead[off[d] + m[:-1]] = 1
        for _, (a, b) in pretok.pre_tokenize_str(text):
            st[off[d] + m[a]] = 1
            en[off[d] + m[b]] = 1
    return st, en, lead


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n]


def _run_core(lib, buf, off):
    jb = load_tokenizer_json(NAME).encode("utf-8")
    n, nd = int(off[-1]), len(off) - 1
    nw = (n >> 6) + 1
    st, en, ld = np.zeros(nw, dtype=np.uint64), np.zeros(nw, dtype=np.uint64), np.zeros(nw, dtype=np.uint64)
    assert lib.clh_run(jb, len(jb), buf.ctypes.data, n, off.ctypes.data, nd, st.ctypes.data, en.ctypes.data, ld.ctypes.data) == 0
    assert not _bits(st, 64 * nw)[n:].any() and not _bits(ld, 64 * nw)[n:].any() and not _bits(en, 64 * nw)[n + 1:].any(), "bits behind the text's end"
    return _bits(st, n + 1), _bits(en, n + 1), _bits(ld, n + 1)


def _check(lib, wheel, docs):
    buf, off = _pack(docs)
    got = _run_core(lib, buf, off)
    exp = _expected(wheel.pre_tokenizer, docs, off)
    for what, g, e in zip(("starts", "ends", "lead mask"), got, exp):
        bad = np.nonzero(g != e)[0]
        if len(bad):
            at = int(bad[0])
            d = int(np.searchsorted(off, at, side="right") - 1)
            d = min(d, len(docs) - 1)
            raise AssertionError(f"{what}: {len(bad)} wrong bytes; first at doc {d} byte {at - off[d]}: {docs[d][:80]!r} got={g[at]} wheel={e[at]}")


def test_the_issues_examples(harness, wheel):
    pre = wheel.pre_tokenizer.pre_tokenize_str
    assert [p for p, _ in pre("'red")] == ["'re", "d"] and [p for p, _ in pre("''s")] == ["''", "s"] and [p for p, _ in pre("!'s")] == ["!'", "s"]
    assert [o for _, o in pre("a  1 2\t")] == [(0, 1), (3, 4), (5, 6)]
    assert [o for _, o in pre("i\u0307")] == [(0, 1), (1, 2)]                    # (what U+0130 lowercases to: two pieces)
    _check(harness, wheel, ["'red", "''s", "!'s", "a  1 2\t", "i\u0307", "it's 3pm", "IT'S", "x'S"])


def test_edge_documents_alone_and_in_batches(harness, wheel):
    edge = cc.edge_docs() + cc.run_docs() + cc.last_byte_docs() + cc.added_docs() + cc.norm_docs()
    for d in edge:                                         # alone: at byte 0 of its batch
        _check(harness, wheel, [d])
    _check(harness, wheel, [d for d in edge if len(d) < 2000])
    long_docs = [d for d in edge if len(d) >= 2000]
    for k in range(0, len(long_docs), 5):
        _check(harness, wheel, long_docs[k:k + 5])
    for b in (["1", "", "'s", "", "", "it's", ""], ["", "", "7"], ["x" * 63 + "'", "s" + "y" * 63, "'re"], ["x" * 62 + "it'", "s", " " * 9 + "1"], [" ", "'", " ", " 's", "1 "],
              ["x" * 64, "", " " * 64, "y" * 64], ["x" * 63 + " ", "x" * 64 + " "], ["\u0130" * 32, "\u0130" * 32, "\U0001f601" * 16]):
        _check(harness, wheel, b)


@pytest.mark.parametrize("total", wt.TOTALS)
def test_total_lengths_at_the_workgroup_edge(total, harness, wheel):
    """the text's last word, the position n_bytes and the edge of a workgroup together: one document and two"""
    for docs in wt.batches(total):
        _check(harness, wheel, docs)


def test_exhaustive_short_strings_at_every_word_offset(harness, wheel):
    """every string of length <= 4 over a 9-symbol alphabet, each a document of its own, the batch behind a filler document of 0..63
    bytes: each string meets every offset of a 64-byte mask word.  The wheel is asked once: its answer does not depend on the filler."""
    alphabet = ["a", " ", "'", "s", "r", "e", "1", "!", "é"]
    strings = ["".join(t) for n in range(1, 5) for t in itertools.product(alphabet, repeat=n)]
    buf0, off0 = _pack(strings)
    exp0 = _expected(wheel.pre_tokenizer, strings, off0)
    for shift in range(64):
        buf = np.concatenate([np.full(shift, ord("x"), dtype=np.uint8), buf0])
        off = np.concatenate([[0], off0 + shift]).astype(np.int64)
        got = _run_core(harness, buf, off)
        head_st, head_en = np.zeros(shift, dtype=np.uint8), np.zeros(shift, dtype=np.uint8)
        head_st[:1] = 1
        exp_en = exp0[1].copy()
        if shift:
            exp_en[0] = 1                                   # (the filler's own end)
        for what, g, e in zip(("starts", "ends", "lead"), got, (np.concatenate([head_st, exp0[0]]), np.concatenate([head_en, exp_en]),
                                                                np.concatenate([np.ones(shift, dtype=np.uint8), exp0[2]]))):
            bad = np.nonzero(g != e)[0]
            assert len(bad) == 0, (what, shift, int(bad[0]))
    for sep in ("b", " ", "2", "'"):                       # ... and without document edges between them
        _check(harness, wheel, [sep.join(strings), "x" * 37 + sep.join(reversed(strings))])


def test_seeded_random_documents(harness, wheel):
    for seed in range(3):
        _check(harness, wheel, cc.random_docs(3000, seed=400 + seed))
    _check(harness, wheel, cc.random_docs(20000, seed=420, lo=0, hi=4))
    # long texts in ONE document each: several workgroups of 16,384 bytes
    _check(harness, wheel, ["".join(cc.random_docs(3000, seed=430)), " ".join(cc.prompts(200, seed=431)), "".join(cc.random_docs(500, seed=432, lo=1, hi=3))])


# ---- 3. the normalizer mode against the wheel's chain --------------------------------------------------------------------------------------

def _chain(ref_tokenizers):
    """normalize_str of the chain the mode implements: the file's without its Replace member, which no kernel runs -- it rewrites the \\s
    runs that the pre-tokenizer drops (the four spellings encode alike: tests/test_clip_gpu.py), but normalize_str shows them"""
    return ref_tokenizers.normalizers.Sequence([ref_tokenizers.normalizers.NFC(), ref_tokenizers.normalizers.Lowercase()]).normalize_str


def _normalize(lib, s):
    jb = load_tokenizer_json(NAME).encode("utf-8")
    raw = s.encode("utf-8")
    cap = 3 * len(raw) + 16
    out, src = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32)
    n = lib.clh_normalize(jb, len(jb), raw, len(raw), out.ctypes.data, src.ctypes.data, cap)
    assert n >= 0, (n, s)
    return out[:n].tobytes().decode("utf-8"), src[:n]


def test_every_scalar_nfc_or_lowercase_changes_alone_and_behind_a_base_letter(harness, ref_tokenizers):
    norm = _chain(ref_tokenizers)
    changing = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000 and norm(chr(cp)) != chr(cp)]
    assert len(changing) > 2500 and 0x130 in changing and 0x41 in changing and 0x212A in changing and 0x3A3 in changing
    bad = []
    for cp in changing:
        for s in (chr(cp), "e" + chr(cp), "E" + chr(cp) + "\u0301x", chr(cp) + chr(cp)):
            if _normalize(harness, s)[0] != norm(s):
                bad.append((hex(cp), s))
    assert not bad, (len(bad), bad[:8])
    # ... and every other scalar stays as it is, in blocks (a block of unchanged chars holds no segment longer than one char)
    changed = set(changing)
    rest = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000 and cp not in changed]
    for k in range(0, len(rest), 20):
        s = "".join(chr(cp) for cp in rest[k:k + 20])
        if norm(s) == s:                                    # (marks in a row may reorder: those blocks are held against the wheel below)
            assert _normalize(harness, s)[0] == s, [hex(c) for c in rest[k:k + 20]]
        else:
            assert _normalize(harness, s)[0] == norm(s), [hex(c) for c in rest[k:k + 20]]


def test_case_documents_text_and_alignment(harness, ref_tokenizers):
    """the text against normalize_str; the alignment against a file of the same chain whose pre-tokenizer isolates every normalized char"""
    norm = _chain(ref_tokenizers)
    iso = ref_tokenizers.Tokenizer.from_str(json.dumps({
        "version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": _seq_norm(cc.NFC, cc.LOWER),
        "pre_tokenizer": {"type": "Split", "pattern": {"Regex": "."}, "behavior": "Isolated", "invert": False},
        "post_processor": None, "decoder": None, "model": {"type": "WordLevel", "vocab": {"<unk>": 0}, "unk_token": "<unk>"}}))
    docs = cc.norm_docs() + cc.last_byte_docs() + cc.random_docs(3000, seed=41, atoms=[a for a in cc.ATOMS if a not in cc.WHITESPACE and a.strip()] + [" "])
    assert _normalize(harness, "\u0130")[0] == "i\u0307" and _normalize(harness, "x\u0130y")[1].tolist() == [0, 1, 1, 1, 3]
    assert _normalize(harness, "I\u0307")[0] == "i\u0307" and _normalize(harness, "Å")[0] == "å" and _normalize(harness, "Σ")[0] == "σ"
    for s, e in zip(docs, iso.encode_batch(docs, add_special_tokens=False)):
        want = norm(s)
        text, src = _normalize(harness, s)
        assert text == want, [hex(ord(c)) for c in s[:40]]
        to_byte = [0]
        for ch in s:
            to_byte.append(to_byte[-1] + len(ch.encode("utf-8")))
        assert len(e.offsets) == len(want)
        exp = []
        for ch, (a, _) in zip(want, e.offsets):
            exp += [to_byte[a]] * len(ch.encode("utf-8"))
        assert src.tolist() == exp, [hex(ord(c)) for c in s[:40]]


def test_the_48_mark_refusal_stays(harness):
    jb = load_tokenizer_json(NAME).encode("utf-8")
    marks = "".join(chr(0x300 + (11 * k) % 0x30) for k in range(60))
    out, src = np.zeros(4000, np.uint8), np.zeros(4000, np.uint32)
    for s, want in (("x E" + marks[:46] + " y", True), ("x E" + marks + " y", False)):
        raw = s.encode("utf-8")
        n = harness.clh_normalize(jb, len(jb), raw, len(raw), out.ctypes.data, src.ctypes.data, 4000)
        assert (n >= 0) == want and (want or n == -2)


# ---- 4. the whole device path under the SIMT emulation -------------------------------------------------------------------------------------

@pytest.fixture()
def simt_library():
    """ctypes opens the host build of the kernels for this test (tests/test_simt_pipeline.py)"""
    from tests.harness import simt_build
    from tokenizers_amd import _lib
    so = simt_build.build()
    saved = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = so, None
    try:
        yield
    finally:
        _lib.LIB_PATH, _lib._lib = saved


def test_the_whole_path_under_the_simt_emulation(simt_library, ref_tokenizers):
    from tests import test_clip_gpu as G
    G.test_vectors_every_array()
    G.test_runs_whitespace_only_and_empty_documents()
    G.test_the_last_byte_of_a_word_decides_the_id()
    G.test_added_tokens_through_the_normalizer_and_raw()
    G.test_special_tokens_pairs_and_truncation_77_with_padding()
    G.test_decode_batch_of_the_variant_without_a_normalized_token()
    G.test_live_differential_against_the_wheel(ref_tokenizers)
