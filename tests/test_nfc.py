"""NFC in front of byte-level BPE, the CPU side: which tokenizer.json shapes load and which are refused (by message), and the
host+device core tokenizers_amd/csrc/nfc_core.hpp -- through tests/harness/nfc_harness.cpp, built with g++ -- against the reference
wheel: the normalized text of every scalar alone and behind `a`, of every active scalar behind starters that compose, of all Hangul
L x V and a stride of LV x T, of seeded segments; the alignment of every output byte on the segments; and the quick check, which may
never pass a string the wheel changes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import nfc_cases as nc
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "nfc_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_nfc_harness.so")


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("nfc_core.hpp", "nfc_tables.inc", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.nfch_normalize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nfch_normalize_batch.restype = C.c_int64
    return lib


def run_core(lib, docs):
    """-> (normalized strings, per-document norig arrays, status bytes)"""
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    text = np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy()
    cap = 3 * int(off[-1]) + 64
    out, norig = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint32)
    ooff, st = np.zeros(len(raw) + 1, dtype=np.int64), np.zeros(len(raw), dtype=np.uint8)
    n = lib.nfch_normalize_batch(text.ctypes.data, off.ctypes.data, len(raw), out.ctypes.data, cap, ooff.ctypes.data, norig.ctypes.data, st.ctypes.data)
    assert n >= 0
    ob = out.tobytes()
    return [ob[ooff[i]:ooff[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(raw))], [norig[ooff[i]:ooff[i + 1]] for i in range(len(raw))], st


def must_flag(d):
    """the quick check's exact predicate: a char whose Quick_Check is not Yes, or a non-starter behind one of a higher class"""
    _, flags, _, _ = nc.tables()
    prev = 0
    for c in d:
        f = flags.get(ord(c), 0)
        r = f & 0x3F
        if f & 0x80 or (r and prev > r):
            return True
        prev = r
    return False


def hold_text(lib, nfc, docs, what):
    got, _, st = run_core(lib, docs)
    for d, g, s in zip(docs, got, st):
        assert bool(s & 2) == must_flag(d), (what, "quick check", [hex(ord(c)) for c in d])
        exp = nfc(d)
        assert not s & 1, (what, [hex(ord(c)) for c in d])
        assert g == exp, (what, [hex(ord(c)) for c in d], [hex(ord(c)) for c in g], [hex(ord(c)) for c in exp])
        # the quick check never passes a string the wheel changes
        assert exp == d or s & 2, (what, "quick check passed a string NFC changes", [hex(ord(c)) for c in d])
    return st


@pytest.fixture(scope="module")
def nfc(ref_tokenizers):
    return ref_tokenizers.normalizers.NFC().normalize_str


def test_every_scalar_alone_and_behind_a(harness, nfc):
    cps = nc.scalars()
    st = hold_text(harness, nfc, [chr(c) for c in cps], "alone")
    # alone, the check flags exactly the chars whose quick check is not Yes: nothing else that is NFC on its own
    _, flags, _, _ = nc.tables()
    for c, s in zip(cps, st):
        assert bool(s & 2) == bool(flags.get(c, 0) & 0x80), hex(c)
    hold_text(harness, nfc, ["a" + chr(c) for c in cps], "behind a")


def test_active_scalars_behind_composing_starters(harness, nfc):
    active, _, _, _ = nc.tables()
    for b in nc.composing_starters():
        hold_text(harness, nfc, [chr(b) + chr(c) for c in active], "behind U+%04X" % b)


def test_hangul(harness, nfc):
    hold_text(harness, nfc, [chr(l) + chr(v) for l in range(0x1100, 0x1113) for v in range(0x1161, 0x1176)], "L x V")
    hold_text(harness, nfc, [chr(lv) + chr(t) for lv in range(0xAC00, 0xD7A4, 28 * 7) for t in range(0x11A7, 0x11C4)], "LV x T")
    hold_text(harness, nfc, [chr(lvt) + chr(t) for lvt in range(0xAC01, 0xD7A4, 28 * 37 + 5) for t in (0x11A8, 0x11C2)], "LVT x T")
    hold_text(harness, nfc, ["\u1100" + chr(v) + chr(t) + "z" for v in range(0x1161, 0x1176, 4) for t in range(0x11A8, 0x11C3, 5)], "L V T")


def _wheel_alignments(ref, docs):
    """per document: the char index every byte of the wheel's NFC text is aligned to -- a byte-level tokenizer without merges behind
    NFC yields one token per normalized byte, and its offsets are that byte's alignment"""
    alphabet = sorted(ref.pre_tokenizers.ByteLevel.alphabet())
    tok = ref.Tokenizer(ref.models.BPE(vocab={c: i for i, c in enumerate(alphabet)}, merges=[]))
    tok.normalizer = ref.normalizers.NFC()
    tok.pre_tokenizer = ref.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    return [e.offsets for e in tok.encode_batch(docs, add_special_tokens=False)]


def hold_alignment(lib, ref, docs, what):
    got, norig, st = run_core(lib, docs)
    exp = _wheel_alignments(ref, docs)
    for d, g, al, e, s in zip(docs, got, norig, exp, st):
        assert not s & 1, (what, d)
        m, b = {}, 0
        for i, ch in enumerate(d):
            m[b] = i
            b += len(ch.encode("utf-8"))
        mine = [(m[int(a)], m[int(a)] + 1) for a in al]
        assert mine == [tuple(o) for o in e], (what, [hex(ord(c)) for c in d], [hex(ord(c)) for c in g], mine, e)


def test_alignment_of_the_issue_table(harness, ref_tokenizers):
    """the wheel facts the core must reproduce, and through them that one source char per output byte (norig, and norig_end's rule for
    where its range ends) is all the offsets need"""
    cases = {"xe\u0301y": [(0, 1), (1, 2), (1, 2), (3, 4)], "a\u0301\u0323b": [(0, 1)] * 3 + [(2, 3)] * 2 + [(3, 4)],
             "x\u0958y": [(0, 1)] + [(1, 2)] * 6 + [(2, 3)], "\u0344q": [(0, 1)] * 4 + [(1, 2)], "\u1100\u1161\u11a8z": [(0, 1)] * 3 + [(3, 4)]}
    docs = list(cases)
    assert [[tuple(o) for o in e] for e in _wheel_alignments(ref_tokenizers, docs)] == list(cases.values())
    hold_alignment(harness, ref_tokenizers, docs, "issue table")


def test_random_segments_text_and_alignment(harness, nfc, ref_tokenizers):
    docs = nc.random_segments(60000, seed=11)
    hold_text(harness, nfc, docs, "random segments")
    hold_alignment(harness, ref_tokenizers, docs[:20000], "random segments")
    # several segments in one string, ASCII between them
    joined = ["".join(docs[i + k] + "xy "[k % 3:] for k in range(5)) for i in range(0, 5000, 5)]
    hold_text(harness, nfc, joined, "joined")
    hold_alignment(harness, ref_tokenizers, joined, "joined")


def test_alignment_of_active_scalars_behind_a_few_starters(harness, ref_tokenizers):
    active, _, decomp, _ = nc.tables()
    hold_alignment(harness, ref_tokenizers, [chr(c) for c in sorted(decomp)] + [chr(c) for c in active], "alone")
    for b in (0x61, 0xE9, 0x1EA1, 0x915, 0xAC00, 0x1100, 0x3B1):
        hold_alignment(harness, ref_tokenizers, [chr(b) + chr(c) + "z" for c in active], "behind U+%04X" % b)


def test_segment_bounds(harness, nfc):
    """30 marks: normalized; 48 chars in one segment: still; beyond: refused, by the flag -- never garbage"""
    marks = "".join(chr(0x300 + (7 * k) % 0x30) for k in range(64))
    ok = ["a" + marks[:30], "a" + marks[:47]]
    hold_text(harness, nfc, ok, "long segments")
    _, _, st = run_core(harness, ["a" + marks[:48], "a" + marks[:60], "x" * 40 + marks[:60] + "y" * 40])
    assert [int(s) & 1 for s in st] == [1, 1, 1]


# ---- loading ------------------------------------------------------------------------------------------------------------------------
def _qwen(**kw):
    d = json.loads(load_tokenizer_json("split_qwen2"))
    d.update(kw)
    return json.dumps(d, ensure_ascii=False)


NFC = {"type": "NFC"}
SEQ = {"type": "Sequence", "normalizers": [{"type": "NFC"}]}


@pytest.mark.parametrize("norm", [NFC, SEQ])
@pytest.mark.parametrize("pre", [None, {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
                                 {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}])
def test_nfc_loads_in_front_of_byte_level_bpe(norm, pre):
    kw = {"normalizer": norm}
    if pre:
        kw["pre_tokenizer"] = pre
    tok = ta.Tokenizer.from_str(_qwen(**kw), device=-1)
    assert tok is not None


def test_normalized_added_token_patterns_are_nfc_normalized_at_load():
    d = json.loads(_qwen(normalizer=NFC))
    nxt = max(max(d["model"]["vocab"].values()), max([a["id"] for a in d["added_tokens"]] or [0])) + 1
    d["added_tokens"].append({"id": nxt, "content": "cafe\u0301", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False})
    assert ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=-1) is not None
    d["added_tokens"][-1]["content"] = "a" + "\u0301" * 60
    with pytest.raises(ta.UnsupportedError, match="more than 48 combining characters"):
        ta.Tokenizer.from_str(json.dumps(d, ensure_ascii=False), device=-1)


WL = {"type": "WordLevel", "vocab": {"<unk>": 0, "a": 1}, "unk_token": "<unk>"}
WP = {"type": "WordPiece", "vocab": {"[UNK]": 0, "a": 1}, "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100}
CBPE = {"type": "BPE", "vocab": {"<unk>": 0, "a": 1}, "merges": [], "unk_token": "<unk>"}
WS = {"type": "Whitespace"}


def _other(model, pre, norm):
    return json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": norm, "pre_tokenizer": pre,
                       "post_processor": None, "decoder": None, "model": model})


@pytest.mark.parametrize("js,msg", [
    (_qwen(normalizer={"type": "NFD"}), "normalizer: type 'NFD' is outside the hot path"),
    (_qwen(normalizer={"type": "NFKC"}), "normalizer: type 'NFKC' is outside the hot path"),
    (_qwen(normalizer={"type": "NFKD"}), "normalizer: type 'NFKD' is outside the hot path"),
    (_qwen(normalizer={"type": "Sequence", "normalizers": [{"type": "NFC"}, {"type": "Lowercase"}]}), "NFC inside a longer Sequence"),
    (_qwen(normalizer={"type": "Sequence", "normalizers": [{"type": "NFD"}, {"type": "NFC"}]}), "NFC inside a longer Sequence"),
    (_qwen(normalizer=NFC, pre_tokenizer={"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True}),
     "ByteLevel add_prefix_space behind a normalizer"),
    (_other(WL, WS, NFC), "NFC is only on the path in front of byte-level BPE"),
    (_other(WP, WS, NFC), "NFC is only on the path in front of byte-level BPE"),
    (_other(CBPE, WS, SEQ), "NFC is only on the path in front of byte-level BPE"),
    (_other(CBPE, {"type": "Metaspace", "replacement": "▁", "prepend_scheme": "always", "split": True}, NFC), "Metaspace behind a normalizer"),
])
def test_refusals_by_message(js, msg):
    with pytest.raises(ta.UnsupportedError, match=msg):
        ta.Tokenizer.from_str(js, device=-1)
