"""BLOOM's Sequence[Split(Regex " ?[^(\\s|[.,!?…。，、।۔،])]+", Isolated), ByteLevel(use_regex=false)] (PT_BLOOM), the CPU side: which
tokenizer.json shapes load and which are refused (by message); the class of 39 chars the pattern leaves out, as the core reads it, against
the reference wheel's Split, scalar by scalar; and the host+device core tokenizers_amd/csrc/pretok_bloom_core.hpp -- what every lane of
k_pretok_bloom executes, through tests/harness/bloom_harness.cpp, built with g++ -- against the wheel's own Sequence."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from oracle import synth
from tests import bloom_cases as bc
from tests import word_edge_totals as wt
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "bloom_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_bloom_harness.so")
UC_ONIG_S, UC_BLOOM_X = 4, 128


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("pretok_bloom_core.hpp", "pretok_gpt2_core.hpp", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.blh_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.blh_run.restype = C.c_int
    for fn in (lib.blh_classes, lib.blh_core_class):
        fn.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
        fn.restype = C.c_int
    return lib


def _file(name=bc.NAME, **over):
    d = json.loads(load_tokenizer_json(name))
    d.update(over)
    return json.dumps(d, ensure_ascii=False)


SPLIT = {"type": "Split", "pattern": {"Regex": bc.PATTERN}, "behavior": "Isolated", "invert": False}
BYTELEVEL = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}


def _seq(*members, **over):
    return _file(pre_tokenizer={"type": "Sequence", "pretokenizers": list(members)}, **over)


def _model(**over):
    m = json.loads(load_tokenizer_json(bc.NAME))["model"]
    m.update(over)
    return m


# ---- 1. load and refuse ------------------------------------------------------------------------------------------------------------

def test_the_fixture_loads_as_the_new_kind():
    tok = ta.Tokenizer.from_str(load_tokenizer_json(bc.NAME), device=-1)
    assert tok.info["pre_tokenizer"] == 11 and tok.info["normalizer"] == 0 and tok.info["model"] == 1 and tok.info["add_prefix_space"] == 0


def test_the_fixture_is_blooms_layout():
    d = json.loads(load_tokenizer_json(bc.NAME))
    assert d["normalizer"] is None and d["pre_tokenizer"] == {"type": "Sequence", "pretokenizers": [SPLIT, BYTELEVEL]}
    assert d["post_processor"]["type"] == "ByteLevel" and d["post_processor"]["trim_offsets"] is False and d["decoder"]["type"] == "ByteLevel"


def test_spellings_that_load():
    assert ta.Tokenizer.from_str(_file(normalizer={"type": "Sequence", "normalizers": []}), device=-1).info["pre_tokenizer"] == 11
    assert ta.Tokenizer.from_str(_seq(SPLIT, dict(BYTELEVEL, trim_offsets=False)), device=-1).info["pre_tokenizer"] == 11
    assert ta.Tokenizer.from_str(_seq({k: v for k, v in SPLIT.items() if k != "invert"}, BYTELEVEL), device=-1).info["pre_tokenizer"] == 11


WORDPIECE = {"type": "WordPiece", "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100, "vocab": {"[UNK]": 0, "a": 1}}
REFUSED = [
    (_seq(dict(SPLIT, behavior="MergedWithPrevious"), BYTELEVEL), r"Split with behavior 'MergedWithPrevious' \(only Isolated is on the path\)"),
    (_seq(dict(SPLIT, behavior="Removed"), BYTELEVEL), r"Split with behavior 'Removed' \(only Isolated is on the path\)"),
    (_seq(dict(SPLIT, invert=True), BYTELEVEL), r"Split with behavior 'Isolated' inverted \(only Isolated is on the path\)"),
    (_seq(dict(SPLIT, behavior="Removed", invert=True), BYTELEVEL), "Split with behavior 'Removed' inverted"),
    (_seq(SPLIT, dict(BYTELEVEL, use_regex=True)), r"Sequence\[Split, ByteLevel\(use_regex=true\)\] applies two regexes"),
    (_seq(SPLIT, dict(BYTELEVEL, add_prefix_space=True)), r"Sequence\[Split, ByteLevel\(add_prefix_space=true\)\] \(a prefix space in front of every pre-token\)"),
    (_file(normalizer={"type": "NFC"}), "BLOOM's Split \\+ ByteLevel behind a normalizer is outside the hot path"),
    (_file(normalizer={"type": "Sequence", "normalizers": [{"type": "NFC"}]}), "BLOOM's Split \\+ ByteLevel behind a normalizer"),
    (_file(normalizer={"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None, "lowercase": False}),
     "BLOOM's Split \\+ ByteLevel behind a normalizer"),
    # a pattern one char off is none of BLOOM's: the family's parser reads it and says what it could not read
    (_seq(dict(SPLIT, pattern={"Regex": bc.PATTERN.replace("،", "")}), BYTELEVEL), "Split pattern outside the tiktoken family"),
    (_seq(dict(SPLIT, pattern={"Regex": bc.PATTERN[1:]}), BYTELEVEL), "Split pattern outside the tiktoken family"),
    (_seq(dict(SPLIT, pattern={"Regex": bc.PATTERN + " "}), BYTELEVEL), "Split pattern outside the tiktoken family"),
    (_seq(dict(SPLIT, pattern={"String": bc.PATTERN}), BYTELEVEL), "Split with a String pattern"),
    (_seq(SPLIT, BYTELEVEL, BYTELEVEL), "this Sequence is outside the hot path"),
    (_file(pre_tokenizer=SPLIT), "Split alone is outside the hot path"),
    (_file(model=_model(end_of_word_suffix="</w>")), "byte-level BPE with continuing_subword_prefix / end_of_word_suffix"),
    (_file(model=_model(byte_fallback=True)), "byte-level BPE with byte_fallback"),
    (_file(model=WORDPIECE, added_tokens=[], post_processor=None, decoder=None), "BLOOM's Split \\+ ByteLevel in front of a WordPiece model"),
    (_file(model={"type": "Unigram", "unk_id": 0, "vocab": [["<unk>", 0.0], ["a", -1.0]], "byte_fallback": False}, added_tokens=[], post_processor=None, decoder=None),
     "BLOOM's Split \\+ ByteLevel in front of a Unigram model"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_near_misses_are_refused_by_reason(k):
    js, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        ta.Tokenizer.from_str(js, device=-1)


# ---- 2. the class ----------------------------------------------------------------------------------------------------------------------

def _flags(lib, name):
    jb = load_tokenizer_json(name).encode("utf-8")
    flags = np.zeros(0x110000, dtype=np.uint8)
    assert lib.blh_classes(jb, len(jb), flags.ctypes.data) == 0
    return flags


@pytest.fixture(scope="module")
def wheel_class(ref_tokenizers):
    """for every scalar value: Split(the pattern, Isolated) cuts "a" + c + "a" (a piece begins at c) iff c is outside the class"""
    split = ref_tokenizers.pre_tokenizers.Split(ref_tokenizers.Regex(bc.PATTERN), "isolated")
    cps = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]
    member = np.zeros(0x110000, dtype=bool)
    for k in range(0, len(cps), 0x8000):
        part = cps[k:k + 0x8000]
        for _, (a, _b) in split.pre_tokenize_str("".join("a" + chr(cp) for cp in part) + "a"):
            if a % 2 == 1:
                member[part[a // 2]] = True
    return member


def test_core_class_equals_the_wheels_on_every_scalar(harness, wheel_class):
    jb = load_tokenizer_json(bc.NAME).encode("utf-8")
    x = np.zeros(0x110000, dtype=np.uint8)
    assert harness.blh_core_class(jb, len(jb), x.ctypes.data) == 0
    assert 0x110000 - 0x800 == 1112064
    bad = np.nonzero(wheel_class != (x != 0))[0]
    assert len(bad) == 0, [hex(int(c)) for c in bad[:8]]
    assert sorted(int(c) for c in np.nonzero(wheel_class)[0]) == sorted(ord(c) for c in bc.X39)
    assert not wheel_class[ord("[")] and not wheel_class[ord("]")]


def test_the_flag_is_the_39_and_touches_no_other_handle_and_no_other_bit(harness):
    base, ours = _flags(harness, "split_qwen2"), _flags(harness, bc.NAME)
    assert not (base & UC_BLOOM_X).any()
    assert np.array_equal(base, ours & ~np.uint8(UC_BLOOM_X))
    assert sorted(int(c) for c in np.nonzero(ours & UC_BLOOM_X)[0]) == sorted(ord(c) for c in bc.X39)
    assert sorted(int(c) for c in np.nonzero(base & UC_ONIG_S)[0]) == sorted(ord(c) for c in bc.ONIG_S)


# ---- 3. the core against the wheel's Sequence ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wheel(ref_tokenizers):
    return ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(bc.NAME)).pre_tokenizer


def _pack(docs):
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum(np.asarray([len(r) for r in raw], dtype=np.int64), out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy(), off, raw


def _expected(pretok, docs, off, raw):
    """-> (piece starts, lead bytes), one byte per text byte"""
    n = int(off[-1])
    buf = np.frombuffer(b"".join(raw), dtype=np.uint8)
    lead = ((buf & 0xC0) != 0x80).astype(np.uint8)
    exp = np.zeros(n, dtype=np.uint8)
    for d, text in enumerate(docs):
        if not text:
            continue
        starts = [a for _, (a, _b) in pretok.pre_tokenize_str(text)]
        if len(raw[d]) == len(text):
            exp[int(off[d]) + np.asarray(starts, dtype=np.int64)] = 1
        else:
            m = np.nonzero(lead[off[d]:off[d + 1]])[0]
            exp[int(off[d]) + m[starts]] = 1
    return exp, lead


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n]


def _run_core(lib, buf, off):
    jb = load_tokenizer_json(bc.NAME).encode("utf-8")
    n, nd = int(off[-1]), len(off) - 1
    st, ld = np.zeros((n >> 6) + 1, dtype=np.uint64), np.zeros((n >> 6) + 1, dtype=np.uint64)
    assert lib.blh_run(jb, len(jb), buf.ctypes.data, n, off.ctypes.data, nd, st.ctypes.data, ld.ctypes.data) == 0
    assert not _bits(st, 64 * len(st))[n:].any() and not _bits(ld, 64 * len(ld))[n:].any(), "bits behind the text's end"
    return _bits(st, n), _bits(ld, n), st


def _first_bad(bad, off, docs, got, exp):
    g = int(bad[0])
    d = int(np.searchsorted(off, g, side="right") - 1)
    return f"{len(bad)} wrong bytes; first at doc {d} byte {g - off[d]}: {docs[d][-40:]!r} got={got[g]} wheel={exp[g]}"


def _hold(got, lead, exp, exp_lead, off, docs):
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, _first_bad(bad, off, docs, got, exp)
    bad = np.nonzero(lead != exp_lead)[0]
    assert len(bad) == 0, "lead mask: " + _first_bad(bad, off, docs, lead, exp_lead)


def _check(lib, wheel, docs):
    buf, off, raw = _pack(docs)
    got, lead, _ = _run_core(lib, buf, off)
    exp, exp_lead = _expected(wheel, docs, off, raw)
    _hold(got, lead, exp, exp_lead, off, docs)


def test_table_of_the_issue(harness, wheel, ref_tokenizers):
    split = ref_tokenizers.pre_tokenizers.Split(ref_tokenizers.Regex(bc.PATTERN), "isolated")
    for text, pieces in bc.TABLE:
        assert [p for p, _ in split.pre_tokenize_str(text)] == pieces, text
        assert [text[a:b] for _, (a, b) in wheel.pre_tokenize_str(text)] == pieces, text
    _check(harness, wheel, [t for t, _ in bc.TABLE])


def test_short_documents_alone_and_in_batches(harness, wheel):
    docs = bc.short_docs()
    for d in docs:                                        # alone: at byte 0 of its batch
        _check(harness, wheel, [d])
    _check(harness, wheel, docs)
    for b in bc.batches():
        _check(harness, wheel, b)


def test_short_documents_at_every_word_offset(harness, wheel):
    """the batch behind a filler document of 0..63 bytes: each document meets every offset of a 64-byte mask word.  The wheel is asked
    once: its answer does not depend on the filler."""
    docs = bc.short_docs() + [d for b in bc.batches() for d in b]
    buf0, off0, raw = _pack(docs)
    exp0, lead0 = _expected(wheel, docs, off0, raw)
    for shift in range(64):
        buf = np.concatenate([np.full(shift, ord("x"), dtype=np.uint8), buf0])
        off = np.concatenate([[0], off0 + shift]).astype(np.int64)
        head = np.zeros(shift, dtype=np.uint8)
        head[:1] = 1
        got, lead, _ = _run_core(harness, buf, off)
        _hold(got, lead, np.concatenate([head, exp0]), np.concatenate([np.ones(shift, dtype=np.uint8), lead0]), off, ["x" * shift] + docs)


@pytest.mark.parametrize("edge", bc.EDGES)
def test_constructed_cases_around_every_edge(edge, harness, wheel):
    """each of the 39, a space in front of a class char and a class char in front of an X char at every offset -8..+8 around the edge of
    a mask word, a wavefront and a workgroup; X chars of two and three bytes straddling it.  Every document alone (the edge is the
    text's), and all of one edge behind each other (the documents' own edges fall anywhere)"""
    docs = bc.constructed_docs(edge)
    assert len(docs) == 17 * (39 + 6) + 4 * (3 + 3 + 4 + 4)
    for d in docs:
        _check(harness, wheel, [d])
    if edge < 16384:
        _check(harness, wheel, docs)


def test_device_edge_documents(harness, wheel):
    docs = bc.device_edge_docs()
    for k, d in enumerate(docs):
        assert len(d.encode("utf-8")) == 16384 + 72
        _check(harness, wheel, [d])
        _check(harness, wheel, docs[max(0, k - 1):k + 2])
    _check(harness, wheel, [bc.big_doc(), "", "x ", "y"])


@pytest.mark.parametrize("total", wt.TOTALS)
def test_total_lengths_at_the_workgroup_edge(total, harness, wheel):
    """the text's last word, the position n_bytes and the edge of a workgroup together: one document and two"""
    for docs in wt.batches(total):
        _check(harness, wheel, docs)


def test_300000_random_documents(harness, wheel):
    """the issue's alphabet -- all 39, class chars of one to four bytes, `[` `]`, U+200B, U+0301, many spaces -- nothing excluded"""
    total = 0
    for seed in range(6):
        docs = bc.random_strings(50000, seed=500 + seed, lo=0, hi=32)
        total += len(docs)
        _check(harness, wheel, docs)
    assert total >= 300000
    # long texts in ONE document each: several workgroups of 16384 bytes
    _check(harness, wheel, ["".join(bc.random_strings(3000, seed=530)), bc.mixed_text(40000, seed=5)])
    _check(harness, wheel, synth.gen_lines(2000, text_seed=3) + synth.stress_lines(seed=4, n=500))


def test_standalone_program_under_sanitizers(harness, wheel, tmp_path):
    """the same comparison by the harness built as a program of its own with -fsanitize=address,undefined: no load or shift of the core
    leaves its buffer or its type's range (the text buffer ends with the 64 bytes of pad the device's has, and at most 15 more)"""
    exe = str(tmp_path / "bloom_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DBLOOM_STANDALONE"] + INCS + SRCS + ["-o", exe],
                   check=True)
    (tmp_path / "tok.json").write_bytes(load_tokenizer_json(bc.NAME).encode("utf-8"))
    sets = {"short": bc.short_docs(), "random": bc.random_strings(20000, seed=540), "empty": ["", ""], "nothing": [],
            "workgroup": [d for d in bc.constructed_docs(16384) if "。" in d or "\u0085" in d][:24], "device_edge": bc.device_edge_docs()}
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        sets[f"len{n}"] = [bc._fit("a. 。", n)]
    for name, docs in sets.items():
        buf, off, raw = _pack(docs)
        exp, _ = _expected(wheel, docs, off, raw)
        words = np.zeros((int(off[-1]) >> 6) + 1, dtype="<u8")
        bits = np.packbits(np.concatenate([exp, np.zeros(64 * len(words) - len(exp), dtype=np.uint8)]), bitorder="little")
        (tmp_path / f"{name}.bin").write_bytes(b"".join(raw))
        (tmp_path / f"{name}.off").write_bytes(off.astype("<i8").tobytes())
        (tmp_path / f"{name}.exp").write_bytes(bits.tobytes())
        r = subprocess.run([exe, str(tmp_path / "tok.json"), str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.off"), str(tmp_path / f"{name}.exp")],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{name}: {r.stdout[-500:]}{r.stderr[-3000:]}"
