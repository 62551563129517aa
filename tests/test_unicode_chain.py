"""The NFD / Lowercase / StripAccents normalizer chains (NORM_CHAIN) on the CPU: what loads and what is refused, by message; the host run of
what the device runs -- the per-char tables, and nfc_core.hpp in its NFD mode where NFD stays visible -- through
tests/harness/unicode_chain_harness.cpp, built with g++, and through tkamd_probe_norm_chain, against the reference wheel: every scalar
alone and behind `a`, seeded strings of bases and marks with the alignment of every output byte, segments at the size limit; the
generated mark table."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import unicode_chain_cases as uc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "unicode_chain_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_unicode_chain_harness.so")


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("nfc_core.hpp", "bert_norm_core.hpp", "nfc_tables.inc", "bert_norm_tables.inc", "unicode_mark_ranges.inc",
                                                    "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.uch_load.argtypes = [C.c_char_p, C.c_int64]
    lib.uch_error.restype = C.c_char_p
    lib.uch_nfd_mode.restype = C.c_uint32
    lib.uch_normalize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.uch_normalize_batch.restype = C.c_int64
    return lib


def run_core(lib, chain, docs):
    """-> (normalized strings, per-document norig arrays, status bytes) of the chain's host run, every document a piece of its own"""
    js = uc.file_of(uc.sequence(chain)).encode("utf-8")
    assert lib.uch_load(js, len(js)) == 0, lib.uch_error()
    assert bool(lib.uch_nfd_mode()) == (chain in uc.NFD_VISIBLE)
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    text = np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy()
    cap = 3 * int(off[-1]) + 64
    out, norig = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint32)
    ooff, st = np.zeros(len(raw) + 1, dtype=np.int64), np.zeros(len(raw), dtype=np.uint8)
    n = lib.uch_normalize_batch(text.ctypes.data, off.ctypes.data, len(raw), out.ctypes.data, cap, ooff.ctypes.data, norig.ctypes.data, st.ctypes.data)
    assert n >= 0
    ob = out.tobytes()
    return [ob[ooff[i]:ooff[i + 1]].decode("utf-8") for i in range(len(raw))], [norig[ooff[i]:ooff[i + 1]] for i in range(len(raw))], st


def _load(js):
    return ta.Tokenizer.from_str(js, device=-1)


def _probe(tok, text):
    """(normalized text, per output byte the first byte of its source char)"""
    raw = text.encode("utf-8")
    cap = 3 * len(raw) + 8
    out, src, n = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32), C.c_int64(0)
    assert tok._lib.tkamd_probe_norm_chain(tok._h, raw, len(raw), out.ctypes.data, src.ctypes.data, cap, C.byref(n)) == 0
    return out[:n.value].tobytes(), src[:n.value]


# ---- 1. what loads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(uc.MODELS))
@pytest.mark.parametrize("chain", uc.ACCEPTED)
def test_every_context_free_sequence_loads(chain, model):
    for pre in uc.PRES:
        tok = _load(uc.file_of(uc.sequence(chain), uc.MODELS[model], pre))
        assert tok.info["normalizer"] == 5


@pytest.mark.parametrize("model", sorted(uc.MODELS))
@pytest.mark.parametrize("member", uc.BARE)
def test_bare_members_load(member, model):
    assert _load(uc.file_of(uc.MEMBER[member], uc.MODELS[model])).info["normalizer"] == 5


def test_the_quicktour_file_loads():
    """normalizers.Sequence([NFD(), Lowercase(), StripAccents()]) + Whitespace + BPE(unk_token) + a template: the file the reference's
    quicktour and its BERT-from-scratch pipeline build.  Refused at the normalizer before this family was on the path."""
    d = json.loads(uc.file_of(uc.sequence("NLS"), dict(uc.CBPE, vocab=dict(uc.CBPE["vocab"], **{"[CLS]": 6, "[SEP]": 7}), unk_token="<unk>")))
    d["added_tokens"] = [{"id": i, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}
                         for c, i in (("[CLS]", 6), ("[SEP]", 7))]
    d["post_processor"] = {"type": "TemplateProcessing",
                           "single": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}}],
                           "pair": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}},
                                    {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
                           "special_tokens": {c: {"id": c, "ids": [i], "tokens": [c]} for c, i in (("[CLS]", 6), ("[SEP]", 7))}}
    tok = _load(json.dumps(d))
    assert tok.info["normalizer"] == 5 and tok.info["model"] == 1
    assert _probe(tok, "H\u00e9llo Y'ALL \u0130")[0] == b"hello y'all i"


# ---- 2. what stays refused, by message ----------------------------------------------------------------------------------------------------
BL = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}
MS = {"type": "Metaspace", "replacement": "\u2581", "prepend_scheme": "always", "split": True}
UNI = {"type": "Unigram", "unk_id": 0, "vocab": [["<unk>", 0.0], ["\u2581a", -1.0]], "byte_fallback": False}
REFUSED = [
    (uc.file_of(uc.sequence("SN")), "'StripAccents' in front of 'NFD'"),
    (uc.file_of(uc.sequence("LL")), "'Lowercase' twice in a Sequence"),
    (uc.file_of(uc.sequence("NLSN")), "'NFD' twice in a Sequence"),
    (uc.file_of({"type": "Sequence", "normalizers": [uc.N, {"type": "NFKC"}]}), "'NFKC' next to NFD / Lowercase / StripAccents"),
    (uc.file_of({"type": "Sequence", "normalizers": [uc.L, {"type": "Strip", "strip_left": True, "strip_right": True}]}), "'Strip' next to NFD / Lowercase / StripAccents"),
    (uc.file_of(uc.sequence("NLS"), dict(uc.CBPE, unk_token=None), BL), r"normalizer: this Sequence is outside the hot path in front of pre_tokenizer 'ByteLevel'"),
    (uc.file_of(uc.L, dict(uc.CBPE, unk_token=None), BL), r"normalizer: type 'Lowercase' is outside the hot path in front of pre_tokenizer 'ByteLevel'"),
    (uc.file_of(uc.sequence("NLS"), uc.CBPE, MS), r"normalizer: this Sequence is outside the hot path in front of pre_tokenizer 'Metaspace'"),
    (uc.file_of(uc.sequence("LS"), UNI, MS), r"normalizer: this Sequence is outside the hot path in front of pre_tokenizer 'Metaspace'"),
    (uc.file_of(uc.sequence("LS"), UNI, uc.PRES[0]), "Unigram"),
    (uc.file_of(uc.sequence("LS"), uc.WL, None), r"normalizer: this Sequence is outside the hot path in front of pre_tokenizer 'null'"),
    (uc.file_of(uc.N, dict(uc.CBPE, unk_token=None), BL), r"normalizer: type 'NFD' is outside the hot path in front of pre_tokenizer 'ByteLevel'"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refusals_by_message(k):
    js, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        _load(js)


def test_a_refused_file_leaves_no_normalizer_kind_behind():
    assert _load(uc.file_of(None)).info["normalizer"] == 0
    assert _load(uc.file_of({"type": "BertNormalizer"})).info["normalizer"] == 1


# ---- 3. every scalar, alone and behind `a`, against the wheel -----------------------------------------------------------------------------
def _scalars():
    return [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]


@pytest.mark.parametrize("chain", uc.ACCEPTED)
def test_every_scalar_against_the_wheel(chain, harness, ref_tokenizers):
    """every scalar alone and behind `a`, each a piece of its own: the text of the host run of what the device runs is the wheel's"""
    norm = uc.wheel_normalizer(ref_tokenizers.normalizers, chain).normalize_str
    for lead in ("", "a"):
        docs = [lead + chr(cp) for cp in _scalars()]
        got, _, st = run_core(harness, chain, docs)
        assert not st.any()
        bad = [[hex(ord(c)) for c in d] for d, g in zip(docs, got) if g != norm(d)]
        assert not bad, (chain, lead, len(bad), bad[:8])


# ---- 4. seeded strings: text and alignment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", uc.ACCEPTED)
def test_seeded_strings_text_and_alignment(chain, harness, ref_tokenizers):
    """bases and marks in and out of canonical order: the normalized text, and for every output byte the source char the reference
    aligns it to (a WordLevel file whose pre-tokenizer isolates every char gives the wheel's per-char offsets); the library's probe
    answers what the harness does"""
    norm = uc.wheel_normalizer(ref_tokenizers.normalizers, chain).normalize_str
    wheel = ref_tokenizers.Tokenizer.from_str(uc.char_isolating_file(chain))
    tok = _load(uc.file_of(uc.sequence(chain)))
    strings = uc.seeded_strings(3000, seed=100 + uc.ACCEPTED.index(chain))
    encs = wheel.encode_batch(strings, add_special_tokens=False)
    got, norig, st = run_core(harness, chain, strings)
    assert not st.any()
    for k, (s, e) in enumerate(zip(strings, encs)):
        want = norm(s)
        assert got[k] == want, (chain, [hex(ord(c)) for c in s])
        assert len(e.offsets) == len(want), (chain, s)
        to_byte = [0]
        for ch in s:
            to_byte.append(to_byte[-1] + len(ch.encode("utf-8")))
        exp = []
        for ch, (a, _) in zip(want, e.offsets):
            exp += [to_byte[a]] * len(ch.encode("utf-8"))
        assert norig[k].tolist() == exp, (chain, [hex(ord(c)) for c in s])
        if k % 10 == 0:
            text, src = _probe(tok, s)
            assert text.decode("utf-8") == want and src.tolist() == exp


@pytest.mark.parametrize("chain", uc.NFD_VISIBLE)
def test_segments_of_47_48_and_49_chars(chain, ref_tokenizers):
    """a segment is normalized up to NFC_SEG_MAX = 48 chars and pieces -- a base and 46 or 47 marks, out of order; behind a base that
    decomposes into two pieces, 45 or 46 --; one more refuses the text, by name"""
    norm = uc.wheel_normalizer(ref_tokenizers.normalizers, chain).normalize_str
    tok = _load(uc.file_of(uc.sequence(chain)))
    marks = "".join(chr(0x300 + (11 * k) % 0x30) for k in range(48))
    for base, most in (("E", 47), ("\u00c9", 46)):
        for n in (most - 1, most):
            s = "x " + base + marks[:n] + " y"
            assert _probe(tok, s)[0].decode("utf-8") == norm(s), (base, n)
        raw = ("x " + base + marks[:most + 1] + " y").encode("utf-8")
        out, src, n = np.zeros(400, np.uint8), np.zeros(400, np.uint32), C.c_int64(0)
        assert tok._lib.tkamd_probe_norm_chain(tok._h, raw, len(raw), out.ctypes.data, src.ctypes.data, 400, C.byref(n)) != 0
        assert b"more than 48 combining characters" in tok._lib.tkamd_last_error()
    with pytest.raises(ta.UnsupportedError, match="more than 48 combining characters"):
        _load(uc.file_of(uc.sequence(chain), added=[_added("a" + marks + "\u0301", 4, True)]))


def test_order_without_nfd_matters_and_lowercase_has_no_final_sigma():
    sl, ls = _load(uc.file_of(uc.sequence("SL"))), _load(uc.file_of(uc.sequence("LS")))
    assert _probe(sl, "\u0130")[0] == "i\u0307".encode() and _probe(ls, "\u0130")[0] == b"i"
    assert _probe(_load(uc.file_of(uc.L)), "\u039f\u0394\u039f\u03a3")[0] == "\u03bf\u03b4\u03bf\u03c3".encode()
    # Me and Mc go with StripAccents, where BertNormalizer's strip_accents drops Mn alone
    assert _probe(_load(uc.file_of(uc.S)), "a\u0488\u0903b")[0] == b"ab"


def test_probe_arguments():
    tok = _load(uc.file_of(uc.sequence("NLS")))
    out, src, n = np.zeros(4, np.uint8), np.zeros(4, np.uint32), C.c_int64(0)
    assert tok._lib.tkamd_probe_norm_chain(tok._h, b"\xed\x95\x9c", 3, out.ctypes.data, src.ctypes.data, 4, C.byref(n)) != 0 and n.value == 9
    assert tok._lib.tkamd_probe_norm_chain(tok._h, b"", 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    plain = _load(uc.file_of(None))
    assert plain._lib.tkamd_probe_norm_chain(plain._h, b"a", 1, out.ctypes.data, src.ctypes.data, 4, C.byref(n)) != 0


# ---- 5. added tokens ------------------------------------------------------------------------------------------------------------------------
def _added(content, i, normalized):
    return {"id": i, "content": content, "single_word": False, "lstrip": False, "rstrip": False, "normalized": normalized, "special": False}


def test_normalized_added_tokens_show_their_normalized_form():
    """Encoding.tokens shows an added-token match as the matched slice of the normalized text (Tokenizer._id_to_token); id_to_token keeps
    the content as registered"""
    tok = _load(uc.file_of(uc.sequence("NLS"), added=[_added("Caf\u00e9", 4, True), _added("<Raw>", 5, False), _added("\u0301", 6, True)]))
    shown = tok._id_to_token()
    assert shown[4] == "cafe" and shown[5] == "<Raw>" and tok.id_to_token(4) == "Caf\u00e9"
    assert shown[6] == ""                              # (normalizes to nothing: never matched, as behind BertNormalizer)
    sl = _load(uc.file_of(uc.sequence("SL"), added=[_added("Caf\u00e9", 4, True)]))
    assert sl._id_to_token()[4] == "caf\u00e9"         # (U+00E9 is no mark: StripAccents without NFD leaves it)


def test_runtime_add_tokens_behind_a_chain():
    tok = _load(uc.file_of(uc.sequence("NLS")))
    assert tok.add_tokens(["Na\u00efve"]) == 1
    assert tok.info["normalizer"] == 5 and tok._id_to_token()[tok.token_to_id("Na\u00efve")] == "naive"


# ---- 6. generated data ----------------------------------------------------------------------------------------------------------------------
def test_mark_table_is_what_the_generator_writes_now(ref_tokenizers):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mark_tables
    finally:
        sys.path.pop(0)
    with open(gen_mark_tables.OUT, encoding="utf-8") as fh:
        assert fh.read() == gen_mark_tables.render()
