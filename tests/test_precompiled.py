"""The Precompiled normalizer in front of Unigram, the CPU side: which tokenizer.json shapes load and which are refused (by message),
malformed charsmaps, and the host+device core tokenizers_amd/csrc/precompiled_core.hpp -- through tests/harness/precompiled_harness.cpp,
built with g++ -- against the reference wheel: the normalized text of every scalar alone, behind `a` and in front of U+0301 under both
charsmaps of tests/precompiled_cases.py (which is also the check of csrc/grapheme_tables.inc: a wrong class joins or cuts a cluster and
the whole-cluster lookup shows it), of seeded clusters, and the alignment of every output byte; the Replace(" {2,}") member's inertness
behind WhitespaceSplit by a wheel differential; and the same harness as a stand-alone program under AddressSanitizer."""
import base64
import ctypes as C
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import tokenizers_amd as ta
from tests import precompiled_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "precompiled_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_precompiled_harness.so")
SEP = "\x0b"                      # a Control no charsmap here has a key for: a cluster boundary on both sides, whatever stands there
MAPS = {"adversarial": pc.adversarial_map, "nmt_nfkc_like": pc.nmt_nfkc_like_map}


def _deps():
    return SRCS + [os.path.join(CSRC, f) for f in ("precompiled_core.hpp", "grapheme_tables.inc", "nfc_core.hpp", "tables.hpp", "host_model.hpp")]


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in _deps()):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.pch_load.argtypes = [C.c_char_p, C.c_int64]
    lib.pch_error.restype = C.c_char_p
    lib.pch_growth.restype = C.c_uint32
    lib.pch_normalize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.pch_normalize_batch.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def blobs():
    return {k: pc.build_charsmap(f()) for k, f in MAPS.items()}


def run_core(lib, docs):
    """-> (normalized strings, per-document norig arrays)"""
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    text = np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy()
    cap = 90 * int(off[-1]) + 64
    out, norig, ooff = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint32), np.zeros(len(raw) + 1, dtype=np.int64)
    assert lib.pch_normalize_batch(text.ctypes.data, off.ctypes.data, len(raw), out.ctypes.data, cap, ooff.ctypes.data, norig.ctypes.data) >= 0
    ob = out.tobytes()
    return [ob[ooff[i]:ooff[i + 1]].decode("utf-8") for i in range(len(raw))], [norig[ooff[i]:ooff[i + 1]] for i in range(len(raw))]


def wheel_texts(norm, docs, chunk=4096):
    """normalize_str of every document: joined with SEP, which never joins a cluster and has no key"""
    out = []
    for k in range(0, len(docs), chunk):
        part = norm.normalize_str(SEP.join(docs[k:k + chunk])).split(SEP)
        assert len(part) == len(docs[k:k + chunk])
        out += part
    return out


def hold_text(lib, norm, docs, what):
    got, _ = run_core(lib, docs)
    exp = wheel_texts(norm, docs)
    bad = [(d, g, e) for d, g, e in zip(docs, got, exp) if g != e]
    assert not bad, (what, len(bad), [([hex(ord(c)) for c in d], g, e) for d, g, e in bad[:8]])


def wheel_alignments(ref, blob, docs):
    """per document: the char range every byte of the wheel's normalized text is aligned to -- a byte-level tokenizer without merges
    behind the normalizer yields one token per normalized byte, and its offsets are that byte's alignment"""
    alphabet = sorted(ref.pre_tokenizers.ByteLevel.alphabet())
    tok = ref.Tokenizer(ref.models.BPE(vocab={c: i for i, c in enumerate(alphabet)}, merges=[]))
    tok.normalizer = ref.normalizers.Precompiled(blob)
    tok.pre_tokenizer = ref.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    return [e.offsets for e in tok.encode_batch(docs, add_special_tokens=False)]


def hold_alignment(lib, ref, blob, docs, what):
    _, norig = run_core(lib, docs)
    exp = wheel_alignments(ref, blob, docs)
    for d, al, e in zip(docs, norig, exp):
        m, b = {}, 0
        for i, ch in enumerate(d):
            m[b] = i
            b += len(ch.encode("utf-8"))
        mine = [(m[int(a)], m[int(a)] + 1) for a in al]
        assert mine == [tuple(o) for o in e], (what, [hex(ord(c)) for c in d], mine, e)


def scalars():
    return [c for c in range(1, 0x110000) if not 0xD800 <= c < 0xE000 and chr(c) != SEP]


@pytest.mark.parametrize("which", list(MAPS))
def test_every_scalar_alone_behind_a_and_in_front_of_a_mark(which, harness, blobs, ref_tokenizers):
    assert harness.pch_load(blobs[which], len(blobs[which])) == 0, harness.pch_error()
    norm = ref_tokenizers.normalizers.Precompiled(blobs[which])
    cps = scalars()
    hold_text(harness, norm, [chr(c) for c in cps], "alone")
    hold_text(harness, norm, ["a" + chr(c) for c in cps], "behind a")
    hold_text(harness, norm, [chr(c) + "\u0301" for c in cps], "in front of U+0301")
    # the classes the first three cannot show: a char behind a Prepend, an Extended_Pictographic behind (c) ZWJ, a pair of regional indicators
    hold_text(harness, norm, ["\u0600" + chr(c) for c in cps], "behind U+0600")
    hold_text(harness, norm, ["\u00a9\u200d" + chr(c) for c in cps], "behind (c) ZWJ")
    hold_text(harness, norm, [chr(c) + "\u200d\u00a9" for c in cps if c < 0x800 or 0x2000 <= c < 0x3300 or c >= 0x1F000], "in front of ZWJ (c)")


def seeded_clusters(n, seed):
    rng = random.Random(seed)
    pool = pc.clusters() + ["a", "b", "x", "y", " ", "\t", "\n", "\r", "\x1e", "\u0301", "\u0302", "\u3099", "\u200d", "\u00a9", "\u00e9", "e", "z", "\ufeff", "\u200b", "\u2122",
                            "\ufb03", "\u0600", "\u0e33", "\U0001f600", "\U0001f1e6", "\U0001f1e7", "\u0915", "\u094d", "\u1100", "\u1161", "\u11a8", "\uac00", "\ufdfa", "\u00bd",
                            "\uff21", "\u3000", "\u00a0", "\u4e2d"]
    return ["".join(rng.choice(pool) for _ in range(rng.randint(1, 7))) for _ in range(n)]


@pytest.mark.parametrize("which", list(MAPS))
def test_seeded_clusters_text_and_alignment(which, harness, blobs, ref_tokenizers):
    assert harness.pch_load(blobs[which], len(blobs[which])) == 0, harness.pch_error()
    norm = ref_tokenizers.normalizers.Precompiled(blobs[which])
    docs = [d for d in seeded_clusters(40000, seed=7) if SEP not in d]
    hold_text(harness, norm, docs, "seeded")
    hold_alignment(harness, ref_tokenizers, blobs[which], docs, "seeded")
    docs = [d for d in pc.corpus() if "\x0b" not in d]
    hold_text(harness, norm, docs, "corpus")
    hold_alignment(harness, ref_tokenizers, blobs[which], [d for d in docs if len(d) < 3000], "corpus")


def test_alignment_of_the_issue_table(harness, blobs, ref_tokenizers):
    """the wheel facts the core must reproduce, behind [WhitespaceSplit, Metaspace(always)] as the issue measured them"""
    m = dict(pc.adversarial_map())
    blob = pc.build_charsmap(m)
    ref = ref_tokenizers
    vocab = [("<unk>", 0.0)] + [(p, -1.0) for p in [pc.MS] + list("xyzfib") + ["TM", "\u00e9"]] + [(pc.MS + "b", -0.5)]
    tok = ref.Tokenizer(ref.models.Unigram(vocab, unk_id=0))
    tok.normalizer = ref.normalizers.Sequence([ref.normalizers.Precompiled(blob), ref.normalizers.Replace(ref.Regex(" {2,}"), " ")])
    tok.pre_tokenizer = ref.pre_tokenizers.Sequence([ref.pre_tokenizers.WhitespaceSplit(), ref.pre_tokenizers.Metaspace(replacement=pc.MS, prepend_scheme="always")])
    rows = {"\x1exy": [(0, 1), (0, 1), (1, 2)], "\x1e\x1exyz \ufb03": [(0, 1), (0, 1), (1, 2), (2, 3), (4, 5), (4, 5), (4, 5), (4, 5)],
            "\ufb03\x1ex": [(0, 1), (0, 1), (0, 1), (1, 2), (2, 3)], "x\x1e\x1ey": [(0, 1), (0, 1), (3, 4)],
            "a  \u2122\x1ea\t \u00e9": [(0, 1), (3, 4), (3, 5), (5, 6), (8, 9), (8, 9)]}
    assert [e.offsets for e in tok.encode_batch(list(rows), add_special_tokens=False)] == list(rows.values())
    assert harness.pch_load(blob, len(blob)) == 0
    hold_alignment(harness, ref, blob, list(rows), "issue table")


def test_replace_of_space_runs_is_inert_behind_whitespace_split(ref_tokenizers):
    """the same file with and without the Replace(Regex " {2,}") member: identical arrays on the whole corpus"""
    d = json.loads(pc.tokenizer_json("precompiled_xlmr"))
    w1 = ref_tokenizers.Tokenizer.from_str(json.dumps(d, ensure_ascii=False))
    d["normalizer"] = d["normalizer"]["normalizers"][0]
    w2 = ref_tokenizers.Tokenizer.from_str(json.dumps(d, ensure_ascii=False))
    docs = pc.corpus() + ["a  b   c", "  x  ", "a \t  b", "\u3000\u3000 a  \u00a0 b", "<mask>  a   <mask>   "]
    for a, b, doc in zip(w1.encode_batch(docs, add_special_tokens=False), w2.encode_batch(docs, add_special_tokens=False), docs):
        assert a.ids == b.ids and a.offsets == b.offsets and a.word_ids == b.word_ids, doc[:60]


# ---- loading ------------------------------------------------------------------------------------------------------------------------
def _edit(name="precompiled_xlmr", **kw):
    d = json.loads(pc.tokenizer_json(name))
    for k, v in kw.items():
        d[k] = v
    return json.dumps(d, ensure_ascii=False)


def _pcn(blob=None):
    return {"type": "Precompiled", "precompiled_charsmap": base64.b64encode(blob if blob is not None else pc.build_charsmap(pc.adversarial_map())).decode()}


def _ms(**kw):
    return {"type": "Metaspace", "replacement": pc.MS, **kw}


RSP = {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}
WSMS = {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, _ms(prepend_scheme="always", split=True)]}


@pytest.mark.parametrize("norm", [_pcn(), {"type": "Sequence", "normalizers": [_pcn()]}, {"type": "Sequence", "normalizers": [_pcn(), RSP]}])
@pytest.mark.parametrize("pre", [WSMS, {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, _ms(add_prefix_space=True)]}])
def test_accepted_chained_shapes(norm, pre):
    tok = ta.Tokenizer.from_str(_edit(normalizer=norm, pre_tokenizer=pre), device=-1)
    assert tok.info["model"] == 4 and tok.info["pre_tokenizer"] == 7 and tok.info["normalizer"] == 4


@pytest.mark.parametrize("pre", [_ms(prepend_scheme="always", split=True), _ms(prepend_scheme="first", split=True), _ms(prepend_scheme="never", split=True), _ms(add_prefix_space=True)])
def test_accepted_bare_metaspace_shapes(pre):
    for norm in (_pcn(), {"type": "Sequence", "normalizers": [_pcn()]}):
        assert ta.Tokenizer.from_str(_edit(normalizer=norm, pre_tokenizer=pre), device=-1).info["normalizer"] == 4


def _bpe_file():
    return json.dumps({"version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": _pcn(), "pre_tokenizer": {"type": "Whitespace"},
                       "post_processor": None, "decoder": None, "model": {"type": "BPE", "vocab": {"<unk>": 0, "a": 1}, "merges": [], "unk_token": "<unk>"}})


def _normalized_added():
    d = json.loads(pc.tokenizer_json("precompiled_xlmr"))
    d["added_tokens"].append({"id": len(d["model"]["vocab"]) + 1, "content": "<n>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True, "special": False})
    return json.dumps(d, ensure_ascii=False)


REFUSED = [
    (_edit(normalizer={"type": "Sequence", "normalizers": [_pcn(), RSP]}, pre_tokenizer=_ms(prepend_scheme="always", split=True)), r"normalizer: Replace\(Regex ' \{2,\}' -> ' '\) behind Precompiled is only"),
    (_edit(normalizer=None), r"pre_tokenizer: Sequence\[WhitespaceSplit, Metaspace\] is only on the path behind a Precompiled"),
    (_edit(pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, _ms(prepend_scheme="first", split=True)]}), r"prepend_scheme 'first'"),
    (_edit(pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, _ms(prepend_scheme="never", split=True)]}), r"prepend_scheme 'never'"),
    (_edit(pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, _ms(prepend_scheme="always", split=False)]}), r"whole pieces.*round differently"),
    (_edit(pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "Whitespace"}, _ms(prepend_scheme="always", split=True)]}), r"pre_tokenizer: this Sequence"),
    (_bpe_file(), r"Precompiled is only on the path in front of a Unigram model"),
    (_edit(normalizer={"type": "Sequence", "normalizers": [_pcn(), {"type": "NFKD"}]}), r"normalizer: 'NFKD' behind Precompiled"),
    (_edit(normalizer={"type": "Sequence", "normalizers": [_pcn(), {"type": "Lowercase"}]}), r"normalizer: 'Lowercase' behind Precompiled"),
    (_edit(normalizer={"type": "Sequence", "normalizers": [_pcn(), {"type": "Strip", "strip_left": True, "strip_right": True}]}), r"normalizer: 'Strip' behind Precompiled"),
    (_edit(normalizer={"type": "Sequence", "normalizers": [_pcn(), {"type": "Replace", "pattern": {"Regex": " +"}, "content": " "}]}), r"normalizer: 'Replace' behind Precompiled"),
    (_edit(normalizer={"type": "Sequence", "normalizers": [_pcn(), RSP, RSP]}), r"behind Precompiled in a Sequence"),
    (_edit(normalizer={"type": "Sequence", "normalizers": [RSP, _pcn()]}), r"[Nn]ormalizer"),
    (_normalized_added(), r"added token '<n>' is normalized = true behind the Precompiled normalizer"),
    (_edit(normalizer={"type": "Precompiled", "precompiled_charsmap": ""}), r"normalizer: Precompiled with an empty precompiled_charsmap"),
    (_edit(normalizer={"type": "Precompiled", "precompiled_charsmap": "!!!"}), r"normalizer: Precompiled precompiled_charsmap is not base64"),
    (_edit(normalizer={"type": "Precompiled"}), r"normalizer: Precompiled without a precompiled_charsmap"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refused_at_load_each_with_its_own_message(k):
    js, rx = REFUSED[k]
    with pytest.raises((ta.UnsupportedError, ValueError), match=rx):
        ta.Tokenizer.from_str(js, device=-1)


def malformed_blobs():
    good = pc.build_charsmap(pc.adversarial_map())
    n = struct.unpack("<I", good[:4])[0]
    units = list(struct.unpack("<%dI" % (n // 4), good[4:4 + n]))
    out = {"truncated header": good[:3], "header alone": good[:4], "truncated trie": good[:4 + n // 2], "trie_bytes beyond the blob": struct.pack("<I", len(good)) + good[4:],
           "trie_bytes odd": struct.pack("<I", n - 2) + good[4:], "invalid UTF-8": good + b"\xff\xfe\0", "a surrogate": good + b"\xed\xa0\x80\0"}
    root = (units[0] >> 10) << ((units[0] & 0x200) >> 6)
    child = root ^ ord("a")
    far = list(units)
    far[child] = (far[child] & 0x3FF) | (((child ^ (len(units) + 77)) & 0x1FFFFF) << 10)
    out["a unit pointing outside"] = struct.pack("<I", n) + struct.pack("<%dI" % len(far), *far) + good[4 + n:]
    nxt = child ^ ((units[child] >> 10) << ((units[child] & 0x200) >> 6))
    val = list(units)
    val[nxt] = 0x80000000 | 0x00FFFFFF
    out["a value outside the replacements"] = struct.pack("<I", n) + struct.pack("<%dI" % len(val), *val) + good[4 + n:]
    rootfar = list(units)
    rootfar[0] = (len(units) + 5) << 10
    out["the root pointing outside"] = struct.pack("<I", n) + struct.pack("<%dI" % len(rootfar), *rootfar) + good[4 + n:]
    out["a replacement of 300 bytes"] = pc.build_charsmap({"q": "x" * 300})
    return out


@pytest.mark.parametrize("what", list(malformed_blobs()))
def test_malformed_charsmaps_are_refused(what, harness):
    blob = malformed_blobs()[what]
    with pytest.raises(ta.UnsupportedError, match=r"normalizer: Precompiled"):
        ta.Tokenizer.from_str(_edit(normalizer=_pcn(blob)), device=-1)
    assert harness.pch_load(blob, len(blob)) == -1 and b"normalizer" in harness.pch_error()


def shared_node_blob():
    """darts-clone builds from a DAWG, so two units may lead to ONE node: here the paths E2 84 and F0 9F 98 end in the same node, whose A2
    is a leaf with a replacement of 255 bytes -- U+2122 (3 bytes) and U+1F622 (4 bytes) both become it"""
    good = pc.build_charsmap({"\u2122": "r" * 255, "\U0001f622": "r" * 255, "a": "b"})
    n = struct.unpack("<I", good[:4])[0]
    units = list(struct.unpack("<%dI" % (n // 4), good[4:4 + n]))
    off = lambda u: (u >> 10) << ((u & 0x200) >> 6)

    def walk(key):
        pos, at = off(units[0]), 0
        for c in key:
            at = pos ^ c
            assert units[at] & 0x800000FF == c
            pos = at ^ off(units[at])
        return at, pos
    _, shared = walk(b"\xe2\x84")
    at, _ = walk(b"\xf0\x9f\x98")
    units[at] = 0x98 | ((at ^ shared) << 10)
    assert walk(b"\xf0\x9f\x98")[1] == shared
    return struct.pack("<I", n) + struct.pack("<%dI" % len(units), *units) + good[4 + n:]


def test_the_growth_bound_holds_for_a_charsmap_with_a_shared_node(harness, ref_tokenizers):
    """the bound of the normalized text is taken at the SMALLEST depth a node is reached at, whichever path the loader's walk met first"""
    blob = shared_node_blob()
    assert harness.pch_load(blob, len(blob)) == 0, harness.pch_error()
    g = harness.pch_growth()
    assert g == 85                                                                  # 255 bytes for the 3 of the shorter key
    docs = ["\u2122" * 300, "\U0001f622" * 300, "a\u2122\U0001f622" * 200]
    got, _ = run_core(harness, docs)
    assert got == [ref_tokenizers.normalizers.Precompiled(blob).normalize_str(d) for d in docs]
    for d, o in zip(docs, got):
        assert len(o.encode()) <= g * len(d.encode()), (len(o.encode()), g * len(d.encode()))
    assert ta.Tokenizer.from_str(_edit(normalizer=_pcn(blob)), device=-1).info["normalizer"] == 4


def test_the_probe_of_the_c_abi():
    tok = ta.Tokenizer.from_str(pc.tokenizer_json("precompiled_ms"), device=-1)
    src = "\ufb03\x1ex".encode()
    out, al, n = np.zeros(64, np.uint8), np.zeros(64, np.uint32), C.c_int64(0)
    assert tok._lib.tkamd_probe_precompiled(tok._h, src, len(src), out.ctypes.data, al.ctypes.data, 64, C.byref(n)) == 0
    assert out[:n.value].tobytes() == b"ffix" and al[:n.value].tolist() == [0, 0, 3, 4]
    assert tok._lib.tkamd_probe_precompiled(tok._h, src, len(src), out.ctypes.data, al.ctypes.data, 2, C.byref(n)) != 0 and n.value == 4


def test_the_harness_program_under_address_sanitizer(tmp_path):
    """the core as a stand-alone program with -fsanitize=address,undefined: the malformed blobs and both charsmaps over the edge documents"""
    exe = str(tmp_path / "pch_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPCH_MAIN"] + INCS + SRCS + ["-o", exe], check=True)
    bl = list(malformed_blobs().values()) + [pc.build_charsmap(f()) for f in MAPS.values()] + [shared_node_blob()]
    docs = [d.encode("utf-8") for d in pc.edge_documents() + seeded_clusters(3000, seed=9)] + [b"\xff\xfe", b"a\xcc", b"\xe2\x80", b"\xf0\x9f\x98", b"\x80\x80\x80\x80\x80\x80"]
    data = tmp_path / "cases.bin"
    with open(data, "wb") as fh:
        for items in (bl, docs):
            fh.write(struct.pack("<I", len(items)))
            for b in items:
                fh.write(struct.pack("<I", len(b)) + b)
    r = subprocess.run([exe, str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "loaded 3 " in r.stdout, r.stdout
