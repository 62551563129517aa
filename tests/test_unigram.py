"""Unigram (SentencePiece Viterbi), the CPU side: which tokenizer.json shapes load and which are refused (by message); the scores as the file
spells them; and the host+device core tokenizers_amd/csrc/unigram_core.hpp -- the body the Unigram kernels run -- through
tests/harness/unigram_harness.cpp, built with g++, against the reference wheel's own model.tokenize on seeded random words."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "unigram_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_unigram_harness.so")
NAMES = ["unigram_ms", "unigram_ms_nobytes", "unigram_adv"]
MS = "▁"
MODEL_UNIGRAM, PT_METASPACE = 4, 7
N_WORDS = 100_000


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("unigram_core.hpp", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.unih_load.argtypes = [C.c_char_p, C.c_size_t]
    lib.unih_load.restype = C.c_int
    lib.unih_error.restype = C.c_char_p
    lib.unih_score.argtypes = [C.c_uint32]
    lib.unih_score.restype = C.c_double
    lib.unih_unk_score.restype = C.c_double
    lib.unih_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.unih_encode.restype = C.c_int64
    return lib


def _load(lib, js: str):
    b = js.encode("utf-8")
    assert lib.unih_load(b, len(b)) == 0, lib.unih_error().decode()


def _encode(lib, words):
    """[(ids, (start, end) per token, error bits)] per word: a <0xXX> token reports its whole run, as the reference's Token does"""
    raw = [w.encode("utf-8") for w in words]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in raw])
    text = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8).copy()
    cap = int(off[-1]) + 1
    ids, ends, isb = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    tof, err = np.zeros(len(raw) + 1, np.int64), np.zeros(len(raw) + 1, np.uint32)
    n = lib.unih_encode(text.ctypes.data, off.ctypes.data, len(raw), ids.ctypes.data, ends.ctypes.data, isb.ctypes.data, tof.ctypes.data, err.ctypes.data, cap)
    assert n >= 0
    out = []
    for w in range(len(raw)):
        a, z = int(tof[w]), int(tof[w + 1])
        e, b = ends[a:z].tolist(), isb[a:z].tolist()
        spans, k = [], 0
        while k < len(e):
            s0 = e[k - 1] if k else 0
            if not b[k]:
                spans.append((s0, e[k]))
                k += 1
                continue
            j = k
            while j + 1 < len(e) and b[j + 1]:
                j += 1
            spans += [(s0, e[j])] * (j - k + 1)
            k = j + 1
        out.append((ids[a:z].tolist(), spans, int(err[w])))
    return out


def _random_words(js: str, seed: int, n: int):
    """words made of the vocabulary's own pieces and of chars it lacks, from one char to a few hundred bytes"""
    d = json.loads(js)
    pieces = [p for p, _ in d["model"]["vocab"] if p]
    rng = random.Random(seed)
    extra = ["ꙮ", "😀", "中", "é", "x", "y", "<unk>", "<", "0", MS, "ß", "̀", "🦀"]
    words = []
    for i in range(n):
        k = rng.choice((1, 1, 2, 2, 3, 4, 6, 9)) if i % 50 else rng.randint(10, 60)
        w = "".join(rng.choice(extra) if rng.random() < 0.25 else rng.choice(pieces) for _ in range(k))
        if rng.random() < 0.3:
            w = w[:rng.randint(1, max(1, len(w)))]              # cut inside a piece
        words.append(w or "a")
    return words


@pytest.mark.parametrize("name", NAMES)
def test_core_against_the_wheels_model_tokenize(harness, name, ref_tokenizers):
    js = load_tokenizer_json(name)
    model = ref_tokenizers.Tokenizer.from_str(js).model
    _load(harness, js)
    words = _random_words(js, 500 + NAMES.index(name), N_WORDS)
    got = _encode(harness, words)
    for w, (ids, spans, err) in zip(words, got):
        exp = model.tokenize(w)
        assert err == 0, w
        assert ids == [t.id for t in exp], w
        assert spans == [t.offsets for t in exp], w


def test_known_answers_of_the_issue(harness, ref_tokenizers):
    """the tie rule ("ab" over ▁:-1 a:-1 b:-1 ab:-2 ▁a:-2 is [▁, ab]: the earliest start), the fused literal unk piece (qq<unk> is one token),
    byte tokens with the offsets of the whole run, one unk where a byte piece is missing"""
    def file(vocab, **model):
        return json.dumps({"added_tokens": [], "normalizer": None, "pre_tokenizer": {"type": "Metaspace", "replacement": MS, "prepend_scheme": "always", "split": True},
                           "post_processor": None, "decoder": None, "model": {"type": "Unigram", "unk_id": 0, "vocab": vocab, **model}}, ensure_ascii=False)
    js = file([["<unk>", 0.0], [MS, -1.0], ["a", -1.0], ["b", -1.0], ["ab", -2.0], [MS + "a", -2.0]])
    _load(harness, js)
    (ids, spans, _), (ids2, spans2, _) = _encode(harness, [MS + "ab", "qq<unk>"])
    assert ids == [1, 4] and spans == [(0, 3), (3, 5)]
    assert ids2 == [0] and spans2 == [(0, 7)]
    w = ref_tokenizers.Tokenizer.from_str(js).model
    assert [t.id for t in w.tokenize(MS + "ab")] == ids and [t.id for t in w.tokenize("qq<unk>")] == ids2
    # min_score counts the unk piece's own score: unk_score = -20 - 10, so unk + q = -15 loses to xq = -3; from the minimum of the OTHER
    # pieces (-5 - 10) it would be 0 and win
    js = file([["<unk>", -20.0], [MS, -5.0], ["q", 15.0], ["xq", -3.0]])
    _load(harness, js)
    (ids, spans, _), = _encode(harness, ["xq"])
    assert ids == [3] and spans == [(0, 2)] and harness.unih_unk_score() == -30.0
    assert [t.id for t in ref_tokenizers.Tokenizer.from_str(js).model.tokenize("xq")] == ids
    js = file([["<unk>", 0.0], [MS, -1.0], ["a", -1.0]] + [["<0x%02X>" % b, -3.0] for b in range(256)], byte_fallback=True)
    _load(harness, js)
    (ids, spans, _), = _encode(harness, ["a中é"])
    assert ids == [2] + [3 + b for b in "中é".encode("utf-8")] and spans == [(0, 1)] + [(1, 6)] * 5
    assert [(t.id, t.offsets) for t in ref_tokenizers.Tokenizer.from_str(js).model.tokenize("a中é")] == list(zip(ids, spans))


def test_unk_id_null_is_an_error_only_where_the_unk_node_is_taken(harness, ref_tokenizers):
    d = json.loads(load_tokenizer_json("unigram_adv"))
    d["model"]["unk_id"] = None
    js = json.dumps(d, ensure_ascii=False)
    _load(harness, js)
    model = ref_tokenizers.Tokenizer.from_str(js).model
    words = _random_words(js, 9, 5000)
    for w, (ids, _, err) in zip(words, _encode(harness, words)):
        try:
            exp = [t.id for t in model.tokenize(w)]
        except Exception as e:
            assert "unk_id" in str(e)
            assert err == 1, w
            continue
        assert err == 0 and ids == exp, w


@pytest.mark.parametrize("name", NAMES)
def test_scores_round_trip(harness, name, ref_tokenizers):
    """the f64 the device adds is the one the REFERENCE holds, for every id: the wheel writes its scores back in the shortest spelling that
    round-trips, which Python reads exactly.  That is not always the file's number correctly rounded (strtod, Python's float): the
    reference's JSON reader rounds twice, and the fixtures with 15-17 digit scores hold entries where the two differ by an ulp.
    unk_score = min over ALL - 10.0"""
    js = load_tokenizer_json(name)
    _load(harness, js)
    vocab = json.loads(js)["model"]["vocab"]
    held = json.loads(ref_tokenizers.Tokenizer.from_str(js).to_str())["model"]["vocab"]
    assert [p for p, _ in held] == [p for p, _ in vocab]
    for i, (_, s) in enumerate(held):
        assert harness.unih_score(i) == float(s), (i, vocab[i])
    assert harness.unih_unk_score() == min(float(s) for _, s in held) - 10.0
    if name != "unigram_adv":
        assert any(len(repr(abs(float(s))).replace(".", "").lstrip("0")) >= 15 for _, s in vocab)
        assert sum(1 for (_, a), (_, b) in zip(vocab, held) if float(a) != float(b)) > 20      # (the fixture does hold such entries)


def test_number_spellings_round_like_the_reference(harness, ref_tokenizers):
    """integers, exponents, more digits than a u64 holds, in front of and behind the point"""
    nums = ["0", "-0", "-0.0", "7", "-3", "1e2", "-1.5E-3", "2.5e+3", "0.1", "-0.30000000000000004", "123456789012345678901234567890", "-18446744073709551616",
            "18446744073709551615.5", "0.123456789012345678901234567890", "-1234567.890123456789012345e-7", "9007199254740993", "-9223372036854775809",
            "1e-320", "4.9e-324", "1.7976931348623157e308", "-123456789012345678.9e-30", "100000000000000000000000e-23"]
    vocab = "[[\"<unk>\", 0.0], [\"▁\", -1.0]" + "".join(', ["p%d", %s]' % (i, s) for i, s in enumerate(nums)) + "]"
    js = json.loads(load_tokenizer_json("unigram_adv"))
    js["model"].update(vocab="@@", unk_id=0)
    js["added_tokens"], js["post_processor"] = [], None
    text = json.dumps(js, ensure_ascii=False).replace('"@@"', vocab)
    _load(harness, text)
    held = json.loads(ref_tokenizers.Tokenizer.from_str(text).to_str())["model"]["vocab"]
    for i, s in enumerate(nums):
        assert harness.unih_score(2 + i) == float(held[2 + i][1]), s


def test_standalone_program_under_sanitizers(tmp_path, ref_tokenizers):
    """the same core as a program of its own with -fsanitize=address,undefined over exact-size buffers: no probe, state access or byte read
    leaves the word; its output is the wheel's"""
    exe = str(tmp_path / "unigram_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DUNIH_MAIN"] + INCS + SRCS + ["-o", exe], check=True)
    for name in ("unigram_ms", "unigram_adv"):
        js = load_tokenizer_json(name)
        words = [w for w in _random_words(js, 77, 3000) if "\n" not in w] + ["a" * 9000, "中" * 3000, "ꙮ" * 700]
        (tmp_path / "tok.json").write_text(js, encoding="utf-8")
        (tmp_path / "words.txt").write_text("\n".join(words) + "\n", encoding="utf-8")
        r = subprocess.run([exe, str(tmp_path / "tok.json"), str(tmp_path / "words.txt")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-300:] + r.stderr[-3000:]
        model = ref_tokenizers.Tokenizer.from_str(js).model
        lines = r.stdout.splitlines()
        assert len(lines) == len(words)
        for w, line in zip(words, lines):
            f = line.split()
            assert f[0] == "0" and [int(x.split(":")[0]) for x in f[1:]] == [t.id for t in model.tokenize(w)], w


# ---- load and refuse (device = -1: the host reader and the tables) ---------------------------------------------------------------------

def _edit(name="unigram_adv", **over):
    d = json.loads(load_tokenizer_json(name))
    for k, v in over.items():
        if k.startswith("model_"):
            d["model"][k[6:]] = v
        else:
            d[k] = v
    return json.dumps(d, ensure_ascii=False)


def _ms(**kw):
    return {"type": "Metaspace", "replacement": MS, **kw}


@pytest.mark.parametrize("name", NAMES)
def test_the_fixtures_load_as_the_new_kind(name):
    tok = ta.Tokenizer.from_str(load_tokenizer_json(name), device=-1)
    d = json.loads(load_tokenizer_json(name))
    assert tok.info["model"] == MODEL_UNIGRAM and tok.info["pre_tokenizer"] == PT_METASPACE and tok.info["normalizer"] == 0
    assert tok.info["vocab_size"] == len(d["model"]["vocab"])                      # the array's length, duplicates and all
    assert tok.get_vocab_size(with_added_tokens=False) == len(d["model"]["vocab"])


@pytest.mark.parametrize("pt", [_ms(prepend_scheme="always", split=True), _ms(prepend_scheme="never", split=True), _ms(prepend_scheme="first", split=True),
                                _ms(prepend_scheme="first"), _ms(add_prefix_space=False), _ms(add_prefix_space=True, split=True)])
def test_accepted_front_shapes(pt):
    for norm in (None, {"type": "Sequence", "normalizers": []}):
        assert ta.Tokenizer.from_str(_edit(pre_tokenizer=pt, normalizer=norm), device=-1).info["model"] == MODEL_UNIGRAM


def test_unk_id_null_and_duplicates_and_added_ids(ref_tokenizers):
    assert ta.Tokenizer.from_str(_edit(model_unk_id=None), device=-1).info["model"] == MODEL_UNIGRAM
    js = load_tokenizer_json("unigram_adv")
    tok, w = ta.Tokenizer.from_str(js, device=-1), ref_tokenizers.Tokenizer.from_str(js)
    assert tok.token_to_id("e") == w.token_to_id("e") == max(i for i, (p, _) in enumerate(json.loads(js)["model"]["vocab"]) if p == "e")
    assert tok.token_to_id("<s>") == w.token_to_id("<s>") and tok.token_to_id("<x>") == w.token_to_id("<x>")
    assert tok.get_vocab_size() == w.get_vocab_size()


REFUSED = [
    (dict(pre_tokenizer=_ms(prepend_scheme="always", split=False)), r"whole pieces.*round differently"),
    (dict(pre_tokenizer=None, normalizer={"type": "Sequence", "normalizers": [{"type": "Prepend", "prepend": MS}, {"type": "Replace", "pattern": {"String": " "}, "content": MS}]}),
     r"whole pieces.*round differently"),
    (dict(pre_tokenizer={"type": "Whitespace"}), r"Unigram \(a vocab of scored pieces\).*pre_tokenizer 'Whitespace' is not"),
    (dict(pre_tokenizer={"type": "WhitespaceSplit"}), r"vocab.*pre_tokenizer 'WhitespaceSplit' is not"),
    (dict(pre_tokenizer={"type": "BertPreTokenizer"}), r"vocab.*pre_tokenizer 'BertPreTokenizer' is not"),
    (dict(pre_tokenizer={"type": "ByteLevel", "add_prefix_space": False, "use_regex": True}), r"vocab.*pre_tokenizer 'ByteLevel' is not"),
    (dict(pre_tokenizer=None), r"pre_tokenizer: null"),
    (dict(normalizer={"type": "NFC"}), r"Metaspace behind a normalizer"),
    (dict(normalizer={"type": "Precompiled", "precompiled_charsmap": ""}), r"[Nn]ormalizer"),
    (dict(pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, _ms(prepend_scheme="always", split=True)]}), r"pre_tokenizer"),
    (dict(pre_tokenizer=_ms(prepend_scheme="always", split=True) | {"replacement": "_"}), r"replacement"),
    (dict(model_unk_id=1000), r"unk_id 1000 is beyond the vocab \(UnkIdNotInVocabulary\)"),
    (dict(model_vocab=[]), r"empty vocab"),
    (dict(model_vocab=[["<unk>", 0.0], ["", -1.0]], model_unk_id=0), r"empty piece"),
    (dict(model_vocab=[["<unk>", 0.0], [MS, -1.0], ["<0x41>", -1.0]], model_unk_id=0, model_byte_fallback=True), r"byte_fallback with 1 of the 256"),
    (dict(model_vocab=[["<unk>", 0.0]] + [["<0x%02X>" % b, -1.0] for b in range(256)], model_unk_id=0, model_byte_fallback=True), r"lacks the piece U\+2581"),
    (dict(model_vocab={"a": 0}), r"model\.vocab missing"),
    (dict(model_vocab=[["a"]]), r"not \[piece, score\]"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refused_at_load_each_with_its_own_message(k):
    over, rx = REFUSED[k]
    with pytest.raises((ta.UnsupportedError, ValueError), match=rx):
        ta.Tokenizer.from_str(_edit(**over), device=-1)


def test_metaspace_decoder_stays_refused_and_served_decoders_build():
    tok = ta.Tokenizer.from_str(_edit(decoder={"type": "Metaspace", "replacement": MS, "prepend_scheme": "always", "split": True}), device=-1)
    assert tok.info["model"] == MODEL_UNIGRAM                                      # (loads: only decode_batch refuses, at the call)
    assert ta.Tokenizer.from_str(load_tokenizer_json("unigram_ms"), device=-1).info["model"] == MODEL_UNIGRAM
