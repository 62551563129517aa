"""The NFKC normalizer in front of the "▁" front (NORM_NFKC) on the CPU: what loads and what stays refused, by message; the host run of
the very core the kernels run -- the K mode of tokenizers_amd/csrc/nfc_core.hpp -- through tkamd_probe_nfkc against the reference
wheel: every scalar alone, every case document and seeded strings with the alignment of every output byte; the count pass against the
write pass through the stand-alone tests/harness/nfkc_harness.cpp, built with g++; the generated tables."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import nfkc_cases as kc
from tests import unicode_chain_cases as uc
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "nfkc_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
EXE = os.path.join(HERE, "harness", "_nfkc_harness")


def _load(js):
    return ta.Tokenizer.from_str(js, device=-1)


@pytest.fixture(scope="module")
def tok():
    return _load(kc.file_of())


def _probe(tok, text):
    """(normalized text, per output byte the first byte of its source char)"""
    raw = text.encode("utf-8")
    cap = 11 * len(raw) + 8
    out, src, n = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32), C.c_int64(0)
    assert tok._lib.tkamd_probe_nfkc(tok._h, raw, len(raw), out.ctypes.data, src.ctypes.data, cap, C.byref(n)) == 0, (text, tok._lib.tkamd_last_error())
    return out[:n.value].tobytes(), src[:n.value]


# ---- 1. what loads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nfkc_spm_bpe", "nfkc_unigram"])
def test_fixtures_load(name):
    """the file the reference's SentencePieceBPETokenizer class builds, and Sequence[NFKC] in front of Unigram: refused at the normalizer
    before NFKC was on the path"""
    t = _load(load_tokenizer_json(name))
    assert t.info["normalizer"] == 6 and t.info["pre_tokenizer"] == 7


@pytest.mark.parametrize("model", sorted(kc.MODELS))
@pytest.mark.parametrize("norm", [kc.K, {"type": "Sequence", "normalizers": [kc.K]}])
def test_every_prepend_scheme_loads(norm, model):
    for pre in (dict(kc.MS, prepend_scheme="always"), dict(kc.MS, prepend_scheme="first"), dict(kc.MS, prepend_scheme="never"),
                {"type": "Metaspace", "replacement": "\u2581", "add_prefix_space": False}):
        assert _load(kc.file_of(norm, kc.MODELS[model], pre)).info["normalizer"] == 6


def test_bpe_options_behind_the_front_load():
    for opts in ({"fuse_unk": True}, {"ignore_merges": True}):
        assert _load(kc.file_of(model=dict(kc.CBPE, **opts))).info["normalizer"] == 6
    vocab = dict(kc.CBPE["vocab"])
    for byte in range(256):
        vocab["<0x%02X>" % byte] = len(vocab)
    assert _load(kc.file_of(model=dict(kc.CBPE, vocab=vocab, byte_fallback=True))).info["normalizer"] == 6


# ---- 2. what stays refused, by message ----------------------------------------------------------------------------------------------------
BL = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}
PINNED = "normalizer: type 'NFKC' is outside the hot path"
NMT_CHAIN = {"type": "Sequence", "normalizers": [{"type": "Nmt"}, kc.K, {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}]}
REFUSED = [
    (kc.file_of(kc.K, dict(uc.CBPE, unk_token=None), BL), PINNED),
    (kc.file_of(kc.K, uc.WL, uc.PRES[0]), PINNED),
    (kc.file_of(kc.K, uc.WP, uc.PRES[2]), PINNED),
    (kc.file_of(kc.K, uc.CBPE, uc.PRES[1]), PINNED),
    (kc.file_of(kc.K, kc.CBPE, None), PINNED),
    (kc.file_of({"type": "Sequence", "normalizers": [kc.K]}, uc.WL, uc.PRES[0]), PINNED),
    (kc.file_of({"type": "NFKD"}), "normalizer: type 'NFKD' is outside the hot path"),
    (kc.file_of({"type": "NFKD"}, uc.WL, uc.PRES[0]), "normalizer: type 'NFKD' is outside the hot path"),
    (kc.file_of(NMT_CHAIN), r"normalizer: 'Nmt' next to NFKC in a Sequence is outside the hot path \(only NFKC alone, or Sequence\[NFKC\], is on it\)"),
    (kc.file_of(NMT_CHAIN, kc.UNI), "'Nmt' next to NFKC in a Sequence"),
    (kc.file_of({"type": "Sequence", "normalizers": [kc.K, {"type": "Strip", "strip_left": True, "strip_right": True}]}), "'Strip' next to NFKC in a Sequence"),
    (kc.file_of({"type": "Sequence", "normalizers": [kc.K, kc.K]}), "'NFKC' twice in a Sequence"),
    (kc.file_of({"type": "Sequence", "normalizers": [kc.K, uc.L]}), "'NFKC' next to NFD / Lowercase / StripAccents"),
    (kc.file_of(pre=dict(kc.MS, split=False)), r"pre_tokenizer: Metaspace\(split = false\) behind NFKC is outside the hot path"),
    (kc.file_of(model=kc.UNI, pre=dict(kc.MS, split=False)), r"pre_tokenizer: Metaspace\(split = false\) behind NFKC is outside the hot path"),
    (kc.file_of({"type": "NFC"}), "pre_tokenizer: Metaspace behind a normalizer"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refusals_by_message(k):
    js, msg = REFUSED[k]
    with pytest.raises(ta.UnsupportedError, match=msg):
        _load(js)


# ---- 3. the probe against the wheel ---------------------------------------------------------------------------------------------------------
def test_every_scalar_alone_against_the_wheel(tok, ref_tokenizers):
    norm = ref_tokenizers.normalizers.NFKC().normalize_str
    bad = []
    for cp in range(0x110000):
        if 0xD800 <= cp < 0xE000:
            continue
        if _probe(tok, chr(cp))[0].decode("utf-8") != norm(chr(cp)):
            bad.append(hex(cp))
    assert not bad, (len(bad), bad[:8])


def _alignment(wheel, docs):
    """per document the byte alignment the wheel's NormalizedString gives its NFKC form: a file whose pre-tokenizer isolates every
    normalized char reports the source range of each as its offsets"""
    out = []
    for s, e in zip(docs, wheel.encode_batch(docs, add_special_tokens=False)):
        to_byte = [0]
        for ch in s:
            to_byte.append(to_byte[-1] + len(ch.encode("utf-8")))
        out.append((e, to_byte))
    return out


def test_case_documents_and_seeded_strings_text_and_alignment(tok, ref_tokenizers):
    norm = ref_tokenizers.normalizers.NFKC().normalize_str
    wheel = ref_tokenizers.Tokenizer.from_str(kc.char_isolating_file())
    docs = kc.edge_docs() + kc.seeded_strings(3000, seed=41)
    docs += [" ".join(kc.seeded_strings(6, seed=7000 + k)) for k in range(300)]
    for s, (e, to_byte) in zip(docs, _alignment(wheel, docs)):
        want = norm(s)
        text, src = _probe(tok, s)
        assert text.decode("utf-8") == want, [hex(ord(c)) for c in s[:40]]
        if "\n" in s or "\r" in s:
            continue                                        # (the isolating pattern `.` does not match a line break: the text alone)
        assert len(e.offsets) == len(want)
        exp = []
        for ch, (a, _) in zip(want, e.offsets):
            exp += [to_byte[a]] * len(ch.encode("utf-8"))
        assert src.tolist() == exp, [hex(ord(c)) for c in s[:40]]


def test_the_issue_table(tok):
    assert _probe(tok, kc.FI)[0] == b"fi" and _probe(tok, kc.FI + "x")[1].tolist() == [0, 0, 3]
    assert _probe(tok, kc.FW_A * 200)[0] == b"A" * 200
    assert _probe(tok, "a" + kc.IDSP + kc.NBSP)[0] == b"a  "
    assert len(_probe(tok, kc.SALLA)[0]) == 33 and set(_probe(tok, "ab" + kc.SALLA)[1].tolist()[2:]) == {2}
    assert _probe(tok, kc.LONG_S)[0] == "\u1e69".encode("utf-8")
    assert _probe(tok, kc.JAMO)[0] == "\uac01".encode("utf-8") and _probe(tok, kc.E_ACUTE)[0] == "\u00e9".encode("utf-8")


def test_segments_at_the_size_limit_and_long_runs(tok, ref_tokenizers):
    """a base and 47 marks normalize, one more is refused by name; hundreds of chars that change on their own are cut by the head rule"""
    norm = ref_tokenizers.normalizers.NFKC().normalize_str
    marks = "".join(chr(0x300 + (11 * k) % 0x30) for k in range(48))
    for base in ("E", kc.FW_A):
        s = "x " + base + marks[:46] + " y"
        assert _probe(tok, s)[0].decode("utf-8") == norm(s)
    raw = ("x E" + uc.MARKS60 + " y").encode("utf-8")
    out, src, n = np.zeros(2000, np.uint8), np.zeros(2000, np.uint32), C.c_int64(0)
    assert tok._lib.tkamd_probe_nfkc(tok._h, raw, len(raw), out.ctypes.data, src.ctypes.data, 2000, C.byref(n)) != 0
    assert b"more than 48 combining characters" in tok._lib.tkamd_last_error()
    for d in kc.long_run_docs():
        assert _probe(tok, d)[0].decode("utf-8") == norm(d)
    with pytest.raises(ta.UnsupportedError, match="more than 48 combining characters"):
        _load(kc.file_of(added=[_added("a" + uc.MARKS60, 10, True)]))


def test_probe_arguments(tok):
    out, src, n = np.zeros(4, np.uint8), np.zeros(4, np.uint32), C.c_int64(0)
    assert tok._lib.tkamd_probe_nfkc(tok._h, kc.SALLA.encode("utf-8"), 3, out.ctypes.data, src.ctypes.data, 4, C.byref(n)) != 0 and n.value == 33
    assert tok._lib.tkamd_probe_nfkc(tok._h, b"", 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    plain = _load(kc.file_of(None))
    assert plain.info["normalizer"] == 0
    assert plain._lib.tkamd_probe_nfkc(plain._h, b"a", 1, out.ctypes.data, src.ctypes.data, 4, C.byref(n)) != 0


# ---- 4. added tokens ------------------------------------------------------------------------------------------------------------------------
def _added(content, i, normalized):
    return {"id": i, "content": content, "single_word": False, "lstrip": False, "rstrip": False, "normalized": normalized, "special": False}


def test_normalized_added_tokens_show_their_normalized_form():
    t = _load(kc.file_of(added=[_added(kc.NORM_TOKEN, 10, True), _added("<Raw>", 11, False), _added(kc.FI, 12, True)]))
    shown = t._id_to_token()
    assert shown[10] == "Caf\u00e9" and shown[11] == "<Raw>" and shown[12] == "fi" and t.id_to_token(10) == kc.NORM_TOKEN
    assert t._normalized(kc.FW_A + kc.IDSP + kc.E_ACUTE) == "A \u00e9"


def test_runtime_add_tokens_behind_nfkc():
    t = _load(kc.file_of())
    assert t.add_tokens(["\uff2e\uff41\u00efve"]) == 1
    assert t.info["normalizer"] == 6 and t._id_to_token()[t.token_to_id("\uff2e\uff41\u00efve")] == "Na\u00efve"


# ---- 5. count pass against write pass ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness_exe():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("nfc_core.hpp", "nfc_tables.inc", "nfkc_tables.inc", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        tmp = f"{EXE}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, EXE)
    return EXE


def test_count_pass_sums_equal_write_pass_lengths(harness_exe, tmp_path):
    docs = kc.edge_docs() + kc.seeded_strings(3000, seed=43) + [chr(cp) * 3 for cp in range(0xA0, 0x10000, 7) if not 0xD800 <= cp < 0xE000]
    docs += ["a" + uc.MARKS60]                                 # (refused: counted apart)
    path = tmp_path / "docs.bin"
    with open(path, "wb") as fh:
        for d in docs:
            raw = d.encode("utf-8")
            fh.write(b"%d\n" % len(raw) + raw)
    r = subprocess.run([harness_exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    f = r.stdout.split()
    assert int(f[f.index("documents") + 1]) == len(docs) and int(f[f.index("refused") + 1]) == 1 and int(f[f.index("bad") + 1]) == 0


# ---- 6. generated data ----------------------------------------------------------------------------------------------------------------------
def test_tables_are_what_the_generator_writes_now(ref_tokenizers):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_nfkc_tables
    finally:
        sys.path.pop(0)
    text, figures = gen_nfkc_tables.render()
    with open(gen_nfkc_tables.OUT, encoding="utf-8") as fh:
        assert fh.read() == text
    assert "growth 11" in figures and "longest 18" in figures and "change 4794" in figures and "heads 4725" in figures
    assert json.dumps(figures)
