"""CPU test of the hot-word table's builder, csrc/hot_table_core.hpp, through the stand-alone program tests/harness/hot_table_harness.cpp
(built with -fsanitize=address,undefined and run as one).  The words come from the committed tokenizers; which of them are ELIGIBLE --
settled, <= 12 bytes: for byte-level BPE a load-time proof by the device merge kernel -- is the recorded fixture
tests/golden/hot_table_eligible.json (tools/make_golden_hot_table.py), next to the SHA-256 of the table a handle builds at load.

  * with every weight equal the builder's table is, byte for byte, the table of the rule it replaced (the lowest ids; a bucket nothing fits
    loses its highest id) and the recorded load-time table: nothing moves before a census has run;
  * with weights from a count of whole pre-tokens, every placed word is found again through hot_hash / hot_bucket / hot_slot (computed here,
    in Python, from the table's bytes), nothing else is in the table, and the placed set is the heaviest words -- ties to the lower id --
    less only words that share a bucket with a placed word or were dropped from one nothing fitted."""
import collections
import hashlib
import json
import os
import shutil
import struct
import subprocess

import pytest

from tests import hot_census_ref as R
from tests.helpers import GOLD, load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "harness", "hot_table_harness.cpp")
NAMES = ["gpt2_synth_50257", "bert_wordpiece_30522", "llama3_128k"]
M = 0xFFFFFFFF


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler here")
    exe = str(tmp_path_factory.mktemp("hot") / "hot_table_harness")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLD, "hot_table_eligible.json"), encoding="utf-8") as fh:
        return json.load(fh)


_words_cache = {}


def eligible_words(name, rec):
    """[(k0, k1, k2, len, id)] of the tokenizer's eligible words, ascending ids"""
    if name not in _words_cache:
        bits = bytes.fromhex(rec["eligible"])
        tb = R.token_bytes(load_tokenizer_json(name))
        out = []
        for i in sorted(tb):
            if i >> 3 < len(bits) and bits[i >> 3] >> (i & 7) & 1:
                b = tb[i]
                assert 1 <= len(b) <= 12, (i, b)
                out.append(struct.unpack("<III", b.ljust(12, b"\0")) + (len(b), i))
        assert len(out) == rec["n_eligible"]
        _words_cache[name] = out
    return _words_cache[name]


def run(exe, mode, slots, seed, words, weights):
    text = "%d %d %d\n" % (slots, seed, len(words)) + "".join("%d %d %d %d %d %d\n" % (w + (wt,)) for w, wt in zip(words, weights))
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    f = dict(l.split(" ", 1) if " " in l else (l, "") for l in r.stdout.splitlines())
    return {"n_hot": int(f["n_hot"]), "weight": int(f["weight"]), "blob": bytes.fromhex(f["blob"]), "placed": [int(x) for x in f["placed"].split()]}


def hot_hash(k0, k1, k2, ln, seed):
    h = (((k0 + seed) & M) * 0x9E3779B1 & M) ^ (((k1 ^ seed) * 0x85EBCA77) & M) ^ ((((k2 + (seed >> 7)) & M) * 0xC2B2AE3D) & M) ^ ((ln * 0x27D4EB2F) & M)
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M
    return h ^ (h >> 12)


def probe(blob, slots, seed, k0, k1, k2, ln):
    """the id the lookup kernel's pass 1 finds for this key in this table, or None"""
    h = hot_hash(k0, k1, k2, ln, seed)
    d = struct.unpack_from("<H", blob, slots * 16 + 2 * (h & (slots // 4 - 1)))[0]
    s = ((h >> 12) + d) & (slots - 1)
    a, b, c, w = struct.unpack_from("<IIII", blob, 16 * s)
    return (w & 0xFFFFFF) if (a, b, c, w >> 24) == (k0, k1, k2, ln) else None


@pytest.mark.parametrize("name", NAMES)
def test_equal_weights_reproduce_the_load_time_table(name, harness, recorded):
    rec = recorded[name]
    words = eligible_words(name, rec)
    core = run(harness, "core", rec["slots"], rec["word_seed"], words, [0] * len(words))
    parent = run(harness, "parent", rec["slots"], rec["word_seed"], words, [0] * len(words))
    assert core["blob"] == parent["blob"], "equal weights: not the table of the lowest-id rule"
    assert sorted(core["placed"]) == sorted(parent["placed"]) and core["n_hot"] == parent["n_hot"] == rec["n_hot"]
    assert hashlib.sha256(core["blob"]).hexdigest() == rec["blob_sha256"], "not the table a handle builds at load"
    # (the order the words are given in does not matter)
    again = run(harness, "core", rec["slots"], rec["word_seed"], words[::-1], [7] * len(words))
    assert again["blob"] == core["blob"]


def python_count(name, n_lines=3000):
    """whole pre-tokens of synthetic text by their bytes, counted with the reference's own pre-tokenizer"""
    tokenizers = pytest.importorskip("tokenizers")
    from oracle import synth
    js = load_tokenizer_json(name)
    ref = tokenizers.Tokenizer.from_str(js)
    docs = synth.gen_lines(n_lines, text_seed=100)
    pts, x = R.pretokens(ref, docs)
    return collections.Counter(x[s:e] for s, e in pts if 0 < e - s <= 12)


@pytest.mark.parametrize("name", NAMES)
def test_counted_weights_place_the_heaviest_words_where_the_kernel_finds_them(name, harness, recorded):
    rec = recorded[name]
    slots, seed = rec["slots"], rec["word_seed"]
    words = eligible_words(name, rec)
    cnt = python_count(name)
    key = lambda w: struct.pack("<III", *w[:3])[:w[3]]
    weights = [cnt.get(key(w), 0) for w in words]
    assert sum(1 for x in weights if x) > 200, "the count met too few eligible words to say anything"
    # words that are NOT eligible ride along with huge weights under another length: the builder takes 1..12 bytes only
    extra = [(1, 2, 3, 13, 1 << 20), (4, 5, 6, 0, (1 << 20) + 1), (7, 8, 9, 16, (1 << 20) + 2)]
    got = run(harness, "core", slots, seed, words + extra, weights + [10 ** 9] * 3)
    placed = set(got["placed"])
    assert len(placed) == len(got["placed"]) == got["n_hot"] and max(placed) < len(words), "an ineligible word was placed"
    assert got["weight"] == sum(weights[i] for i in placed)
    # every placed word is found, with its id; every slot of the table is a placed word or empty
    for i in placed:
        assert probe(got["blob"], slots, seed, *words[i][:4]) == words[i][4], words[i]
    filled = sum(1 for s in range(slots) if struct.unpack_from("<I", got["blob"], 16 * s + 12)[0] >> 24)
    assert filled == len(placed)
    # the placed set: the top 15/16 * slots by (weight descending, id ascending), less only words dropped from their bucket
    order = sorted(range(len(words)), key=lambda i: (-weights[i], words[i][4]))
    top = order[:slots * 15 // 16]
    assert placed <= set(top)
    bucket = lambda i: hot_hash(*words[i][:4], seed) & (slots // 4 - 1)
    by_bucket = collections.defaultdict(list)
    for i in top:
        by_bucket[bucket(i)].append(i)
    for b, members in by_bucket.items():          # a bucket keeps a prefix of its words in that order: it only ever loses its lightest
        kept = [i for i in members if i in placed]
        assert kept == members[:len(kept)], (b, members, kept)
    assert len(placed) >= len(top) - 16, "more than a handful of words lost their bucket"
    # and it pays: the weight it holds against the weight the lowest ids hold
    base = run(harness, "core", slots, seed, words, [0] * len(words))
    assert got["weight"] > sum(weights[i] for i in base["placed"])
