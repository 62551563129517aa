"""The chained Split pre-tokenizer of DeepSeek-V3 / R1, the CPU side: which tokenizer.json shapes load and which are refused (by message);
the second class table against the reference wheel's regex engine, scalar by scalar; and the host+device core
tokenizers_amd/csrc/pretok_ds3_core.hpp -- the lane kernel's window function and the sequential matcher, through
tests/harness/ds3_harness.cpp, built with g++ -- against the wheel's own Sequence of Splits."""
import copy
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from oracle import synth
from tests import split_chain_cases as sc
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "ds3_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_ds3_harness.so")
NAME = "ds3_chain"


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("pretok_ds3_core.hpp", "pretok_l3_core.hpp", "unicode_psm_ranges.inc", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.ds3h_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.ds3h_run.restype = C.c_int
    lib.ds3h_seq.argtypes = lib.ds3h_run.argtypes[:-1]
    lib.ds3h_seq.restype = C.c_int
    lib.ds3h_classes.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    lib.ds3h_classes.restype = C.c_int
    return lib


def _file(**over):
    d = json.loads(load_tokenizer_json(NAME))
    d.update(over)
    return json.dumps(d, ensure_ascii=False)


def _chain(edit):
    """the fixture's file with its pre-tokenizer section edited in place by `edit`"""
    d = json.loads(load_tokenizer_json(NAME))
    pt = copy.deepcopy(d["pre_tokenizer"])
    edit(pt["pretokenizers"])
    d["pre_tokenizer"] = pt
    return json.dumps(d, ensure_ascii=False)


def _set(k, path, value):
    def edit(p):
        t = p[k]
        for key in path[:-1]:
            t = t[key]
        t[path[-1]] = value
    return edit


def _rx(k, fn):
    def edit(p):
        p[k]["pattern"]["Regex"] = fn(p[k]["pattern"]["Regex"])
    return edit


# ---- 1. load and refuse ------------------------------------------------------------------------------------------------------------

def test_the_fixture_loads_as_the_new_kind():
    tok = ta.Tokenizer.from_str(load_tokenizer_json(NAME), device=-1)
    assert tok.info["pre_tokenizer"] == 8 and tok.info["normalizer"] == 0 and tok.info["model"] == 1


PUNCT = "!\"#$%&'()*+,\\-./:;<=>?@\\[\\\\\\]^_`{|}~"
SPELLINGS = [
    lambda r: r.replace("\r", "\\r").replace("\n", "\\n"),                               # CR and LF escaped, as the files on the hub print them
    lambda r: r.replace(PUNCT, "!-/:-@\\[-`{-~"),                                         # the class as four ranges
    lambda r: r.replace(PUNCT, "\\!\\\"\\#\\$\\%\\&\\'\\(\\)\\*\\+\\,\\-\\.\\/\\:\\;\\<\\=\\>\\?\\@\\[\\\\\\]\\^\\_\\`\\{\\|\\}\\~"),   # every member escaped
    lambda r: r.replace(PUNCT, "~}|{`_^\\]\\\\\\[@?>=<;:/.\\-,+*)('&%$#\"!"),             # another order
    lambda r: r.replace(PUNCT, "\\x21-\\x2F\\x3a-\\x40\\u005B-\\u0060\\x{7b}-\\x{7E}"),  # numeric escapes
]


@pytest.mark.parametrize("k", range(len(SPELLINGS)))
def test_spellings_of_the_punctuation_class_load(k):
    js = _chain(_rx(2, SPELLINGS[k]))
    assert js != load_tokenizer_json(NAME)
    assert ta.Tokenizer.from_str(js, device=-1).info["pre_tokenizer"] == 8


def test_spellings_of_the_cjk_class_load():
    for rx in ("[\\u4E00-\\u9FA5\\u3040-\\u309F\\u30A0-\\u30FF]+", "[぀-ヿ一-龥]+", "[\\x{3040}-\\x{30ff}\\x{4e00}-\\x{9fa5}]+"):
        assert ta.Tokenizer.from_str(_chain(_set(1, ("pattern", "Regex"), rx)), device=-1).info["pre_tokenizer"] == 8


def test_normalizer_sequence_of_nothing_loads_and_nfc_in_front_too():
    d = json.loads(load_tokenizer_json("split_qwen2"))
    d["normalizer"] = {"type": "Sequence", "normalizers": []}
    assert ta.Tokenizer.from_str(json.dumps(d), device=-1).info["normalizer"] == 0       # (in front of a one-Split member as well)
    assert ta.Tokenizer.from_str(_file(normalizer=None), device=-1).info["normalizer"] == 0
    assert ta.Tokenizer.from_str(_file(normalizer={"type": "NFC"}), device=-1).info["normalizer"] == 3


def _swap(i, j):
    def edit(p):
        p[i], p[j] = p[j], p[i]
    return edit


REFUSED = [
    (_chain(_swap(0, 1)), "the order of the stages"),
    (_chain(_swap(1, 2)), "the order of the stages"),
    (_chain(_swap(0, 2)), "the order of the stages"),
    (_chain(lambda p: p.pop(1)), "a chain of 2 Splits"),
    (_chain(lambda p: p.insert(1, copy.deepcopy(p[1]))), "a chain of 4 Splits"),
    (_chain(_set(0, ("pattern", "Regex"), "\\p{N}{1,2}")), r"digit count '\\p\{N\}\{1,2\}'"),
    (_chain(_set(0, ("pattern", "Regex"), "\\p{N}")), "digit count"),
    (_chain(_set(0, ("pattern", "Regex"), "\\p{N}+")), "digit count"),
    (_chain(_set(1, ("pattern", "Regex"), "[一-龥぀-ゟ゠-ヿ가-힣]+")), r"the CJK class holds U\+AC00"),
    (_chain(_set(1, ("pattern", "Regex"), "[一-龥぀-ゟ゠-ヾ]+")), r"the CJK class lacks U\+30FF"),
    (_chain(_set(1, ("pattern", "Regex"), "[一-龥぀-ゟ゠-ヿ]")), "not a class followed by \\+"),
    (_chain(_set(1, ("pattern", "Regex"), "[^一-龥]+")), "negated class"),
    (_chain(_rx(2, lambda r: r.replace("!\"#", "!\"#§"))), r"the punctuation class holds U\+00A7"),
    (_chain(_rx(2, lambda r: r.replace("!\"#", "!#"))), r"the punctuation class lacks U\+0022"),
    (_chain(_rx(2, lambda r: r.replace("[A-Za-z]+", "[a-z]+"))), r"is not \[punctuation\]\[A-Za-z\]\+"),
    (_chain(_rx(2, lambda r: r.replace("\\p{M}", ""))), "third pattern: alternative"),
    (_chain(_rx(2, lambda r: r + "|x")), "7 alternatives"),
    (_chain(_rx(2, lambda r: r.replace("|\\s+(?!\\S)", ""))), "5 alternatives"),
    (_chain(_set(0, ("behavior",), "Removed")), "chained Split with behavior 'Removed'"),
    (_chain(_set(2, ("behavior",), "MergedWithPrevious")), "chained Split with behavior 'MergedWithPrevious'"),
    (_chain(_set(1, ("invert",), True)), "inverted"),
    (_chain(_set(1, ("pattern",), {"String": "中"})), "chained Split with a String pattern"),
    (_chain(_set(3, ("add_prefix_space",), True)), "add_prefix_space=true"),
    (_chain(_set(3, ("use_regex",), True)), "use_regex=true"),
    (_file(normalizer={"type": "NFKC"}), "normalizer: type 'NFKC' is outside the hot path"),
    (_file(normalizer={"type": "Sequence", "normalizers": [{"type": "NFC"}, {"type": "Lowercase"}]}), "NFC inside a longer Sequence"),
    (_file(normalizer={"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None, "lowercase": False}),
     "the chained Split behind a normalizer other than NFC"),
    (_file(normalizer={"type": "Sequence", "normalizers": [{"type": "Lowercase"}]}), "normalizer: this Sequence is outside the hot path"),
    # out of scope, each with its reason: the older DeepSeek-LLM / Coder chain, Falcon's Punctuation + Digits, a String Split
    (_chain(_rx(2, lambda r: r.replace("|\\s+(?!\\S)|\\s+", "|\\s+$"))), "5 alternatives"),
    (_file(pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "Punctuation", "behavior": "Contiguous"}, {"type": "Digits", "individual_digits": False},
                                                                  {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}]}),
     "pre_tokenizer: this Sequence is outside the hot path"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_near_misses_are_refused_by_reason(k):
    js, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        ta.Tokenizer.from_str(js, device=-1)


# ---- 2. classes ------------------------------------------------------------------------------------------------------------------------

def test_second_class_table_equals_the_wheels_regex_engine(harness, ref_tokenizers):
    """for every scalar value: P / S / M / CJK of the table the loader builds == what Split(Regex(class), removed) removes"""
    jb = load_tokenizer_json(NAME).encode("utf-8")
    flags = np.zeros(0x110000, dtype=np.uint8)
    assert harness.ds3h_classes(jb, len(jb), flags.ctypes.data) == 0
    cps = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]
    assert not flags[0xD800:0xE000].any()
    for bit, rx in ((1, r"\p{P}"), (2, r"\p{S}"), (4, r"\p{M}"), (8, "[一-龥぀-ゟ゠-ヿ]")):
        split = ref_tokenizers.pre_tokenizers.Split(ref_tokenizers.Regex(rx), behavior="removed")
        member = np.ones(0x110000, dtype=bool)
        member[0xD800:0xE000] = False
        for k in range(0, len(cps), 0x8000):
            part = cps[k:k + 0x8000]
            for _, (a, b) in split.pre_tokenize_str("".join(map(chr, part))):
                member[part[a:b]] = False
        bad = np.nonzero(member != ((flags & bit) != 0))[0]
        assert len(bad) == 0, (rx, [hex(int(x)) for x in bad[:8]])
    # ASCII: what the kernel's byte table says without a table load
    for v in range(128):
        assert bool(flags[v] & 3) == (33 <= v < 127 and not chr(v).isalnum()), v


# ---- 3 / 4. the core and the sequential matcher against the wheel's chain -----------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(ref_tokenizers):
    return ref_tokenizers.Tokenizer.from_str(load_tokenizer_json(NAME)).pre_tokenizer


def _pack(docs):
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy(), off


def _expected(chain, docs, off):
    exp = np.zeros(int(off[-1]), dtype=np.uint8)
    for d, text in enumerate(docs):
        if text.isascii():
            for _, (a, _b) in chain.pre_tokenize_str(text):
                exp[off[d] + a] = 1
        else:
            m = np.cumsum([0] + [len(c.encode("utf-8")) for c in text])
            for _, (a, _b) in chain.pre_tokenize_str(text):
                exp[off[d] + m[a]] = 1
    return exp


def _first_bad(bad, off, docs, got, exp):
    g = int(bad[0])
    d = int(np.searchsorted(off, g, side="right") - 1)
    return f"{len(bad)} wrong bytes; first at doc {d} byte {g - off[d]}: {docs[d]!r} got={got[g]} wheel={exp[g]}"


def _run_core(lib, buf, off):
    """-> (window core's starts, its undecided bytes, the sequential matcher's starts), one byte per text byte"""
    jb = load_tokenizer_json(NAME).encode("utf-8")
    n, nd = int(off[-1]), len(off) - 1
    st, un, sq = np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint8)
    assert lib.ds3h_run(jb, len(jb), buf.ctypes.data, n, off.ctypes.data, nd, st.ctypes.data, un.ctypes.data) == 0
    assert lib.ds3h_seq(jb, len(jb), buf.ctypes.data, n, off.ctypes.data, nd, sq.ctypes.data) == 0
    return st[:n], un[:n], sq[:n]


def _hold(st, un, sq, exp, off, docs):
    bad = np.nonzero((un == 0) & (st != exp))[0]
    assert len(bad) == 0, "window core: " + _first_bad(bad, off, docs, st, exp)
    bad = np.nonzero(sq != exp)[0]
    assert len(bad) == 0, "sequential matcher: " + _first_bad(bad, off, docs, sq, exp)


def _check(lib, chain, docs):
    """every byte the window core decides == the wheel; the sequential matcher == the wheel on every byte.  -> undecided share"""
    buf, off = _pack(docs)
    st, un, sq = _run_core(lib, buf, off)
    _hold(st, un, sq, _expected(chain, docs, off), off, docs)
    return float(un.mean()) if len(un) else 0.0


def test_table_of_chain_versus_alternation(harness, chain):
    table = [["a", "  ", "1"], ["  ", "中"], ["中文", "abc", "かな", "1"], ["a", "\u200db", " ", "\x01\x02", " c"], ["x", " .", "b", " ..", "b", " a", ".b", "._", "c"]]
    for text, pieces in zip(sc.TABLE, table):
        assert "".join(pieces) == text
        ends = list(itertools.accumulate(len(p) for p in pieces))
        assert [o for _, o in chain.pre_tokenize_str(text)] == [(e - len(p), e) for p, e in zip(pieces, ends)], text
    _check(harness, chain, sc.TABLE + sc.edge_docs())


def test_exhaustive_short_strings_at_every_window_offset(harness, chain):
    """every string of length <= 5 over the 12-symbol alphabet, each a document of its own, the batch behind a filler document of 0..63
    bytes: each string meets every offset of a 64-byte window (and of a 48-byte lane).  The wheel is asked once: its answer does not
    depend on the filler."""
    strings = ["".join(t) for n in range(1, 6) for t in itertools.product(sc.ALPHABET, repeat=n)]
    assert len(strings) == sum(12 ** n for n in range(1, 6))
    buf0, off0 = _pack(strings)
    exp0 = _expected(chain, strings, off0)
    for shift in range(64):
        buf = np.concatenate([np.full(shift, ord("x"), dtype=np.uint8), buf0])
        off = np.concatenate([[0], off0 + shift]).astype(np.int64)
        head = np.zeros(shift, dtype=np.uint8)
        head[:1] = 1
        st, un, sq = _run_core(harness, buf, off)
        _hold(st, un, sq, np.concatenate([head, exp0]), off, ["x" * shift] + strings)


def test_seeded_random_strings(harness, chain):
    for seed in range(4):
        _check(harness, chain, sc.random_strings(3000, seed=300 + seed))
        _check(harness, chain, sc.random_strings(3000, seed=310 + seed, alphabet=sc.WIDE))
    _check(harness, chain, sc.random_strings(20000, seed=320, lo=0, hi=24, alphabet=sc.WIDE))
    # one long text in ONE document: the same strings without document edges between them
    _check(harness, chain, ["".join(sc.random_strings(400, seed=330, alphabet=sc.WIDE)), sc.big_doc(), sc.mixed_text(5000, seed=5)])


def test_runs_that_end_at_a_window_edge(harness, chain):
    docs = sc.window_edge_runs()
    assert len(docs) > 3000
    _check(harness, chain, docs)
    _check(harness, chain, ["".join(docs[k::97]) for k in range(97)])       # ... and the same runs inside long documents


# ---- 5. the slow tier is not the path -------------------------------------------------------------------------------------------------

def test_prose_is_decided_by_the_window_core(harness, chain):
    """On oracle.synth prose this core leaves at most twice the share of bytes undecided that the Llama-3 core leaves on the same text
    (two more kinds of run -- marks, P / S runs -- can reach a window's edge).  Measured here: see DESIGN.md section 3c."""
    from tests import test_pretok_core as l3t
    docs = synth.gen_lines(20000, text_seed=3) + synth.stress_lines(seed=4, n=3000)
    so = os.path.join(HERE, "harness", "_ds3_l3_harness.so")      # (the Llama-3 core's harness, built here as tests/test_pretok_core.py builds it)
    srcs = [os.path.join(HERE, "harness", "l3_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
    deps = srcs + [os.path.join(CSRC, f) for f in ("pretok_gpt2_core.hpp", "pretok_l3_core.hpp", "pretok_local_core.hpp", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + srcs + ["-o", tmp], check=True)
        os.replace(tmp, so)
    lib3 = C.CDLL(so)
    lib3.l3h_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib3.l3h_run.restype = C.c_int
    js3 = load_tokenizer_json("llama3_small_6000")
    _, un3, _ = l3t._run(lib3, js3, docs)
    share3 = float(un3.mean())
    share = _check(harness, chain, docs)
    print(f"undecided share of bytes: chained Split {share:.6f}, Llama-3 {share3:.6f}")
    assert share3 > 0, "the bound would be vacuous: the Llama-3 core leaves nothing undecided on this text"
    assert share <= 2 * share3, (share, share3)
