"""The hot table's census and rebuild on the CPU: csrc/ compiled for the host under the SIMT shim (like tests/test_simt_pipeline.py), the
census hooks at 0 bytes / period 1 so that every batch of a handle takes a census, a GPT-2 layout (pre-tokens end where the next starts)
and the BERT layout (end masks; behind its normalizer, where the text's length exists on the device only).

  * what k_hot_census counted equals a Python recount of the same sample, made with the reference's own normalizer and pre-tokenizer
    (tests/hot_census_ref.py): texts of 100 bytes, of a tile +- 1 byte, of 40 KB with a pre-token over each tile edge, words of 12 and 13
    bytes, an empty document, a non-ASCII document, and a text of more than 64 tiles (the strided sample);
  * ids, char offsets and word ids of the committed vectors are what they were before the census, on the batch that takes it, and after the
    rebuild;
  * the calls a census batch and its synchronisation enqueue are the recorded ones (tests/golden/launch_sequences_hot_census.json)."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tokenizers_amd import _lib

from tests import hot_census_ref as R
from tests.harness import simt_build
from tests.helpers import GOLD, load_tokenizer_json, load_vectors

FIXTURE = os.path.join(GOLD, "launch_sequences_hot_census.json")
HOOKS = {"TKAMD_TEST_HOOKS": "1", "TKAMD_HOT_CENSUS_MIN_BYTES": "0", "TKAMD_HOT_CENSUS_PERIOD": "1", "TKAMD_PACED": "0"}
TILE = R.TILE


@pytest.fixture(scope="module", autouse=True)
def simt_library():
    simt_build.build()
    saved = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    saved_env = {k: os.environ.get(k) for k in HOOKS}
    os.environ.update(HOOKS)
    try:
        yield
    finally:
        _lib.LIB_PATH, _lib._lib = saved
        for k, v in saved_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _json_of(layout):
    if layout == "gpt2":
        d = json.loads(load_tokenizer_json("bytelevel_prefix_trim_3000"))
        d["pre_tokenizer"]["add_prefix_space"] = False
        d["post_processor"] = None
        return json.dumps(d)
    return load_tokenizer_json("bert_wordpiece_4000")


SENT = "the quick brown fox jumps over the lazy dog and it is not what they said , is it ? "


def _exactly(n):
    """n bytes of ASCII words"""
    return (SENT * (n // len(SENT) + 1))[:n]


def _over_edges():
    """40 KB with one word lying over each of the two tile edges"""
    a = _exactly(TILE - 3) + "overlapping "
    b = _exactly(2 * TILE - 5 - len(a)) + " straddles "
    return a + b + _exactly(40 * 1024 - len(a) - len(b))


TEXTS = {
    "100_bytes": [_exactly(100)],
    "tile_minus_1": [_exactly(TILE - 1)],
    "tile": [_exactly(TILE)],
    "tile_plus_1": [_exactly(TILE + 1)],
    "two_docs_meet_at_a_tile_edge": [_exactly(TILE - 2) + "it", "is it the dog ?"],
    "40k_words_over_tile_edges": [_over_edges()],
    "words_of_12_and_13_bytes": None,          # (from the vocabulary: _words_12_13)
    "empty_documents": ["", "the dog", "", ""],
    "only_empty": [""],
    "non_ascii": ["café naïve 中文 Жук \U0001F600 ok the dog", "über the straße", "the"],
    "more_than_64_tiles": [_exactly(700)] * 1600,
}


def _words_12_13(js, eligible):
    """documents of the vocabulary's own words of 12 bytes (eligible) and of 13 (never): each alone, and all in one line"""
    tb, el = R.token_bytes(js), set(eligible)
    w12 = sorted(b for i, b in tb.items() if len(b) == 12 and i in el and b.strip().isalpha())[:6]
    w13 = sorted(b for b in tb.values() if len(b) == 13 and b.strip().isalpha())[:6]
    assert w12 and w13
    ws = [b.decode() for pair in zip(w12, w13) for b in pair]
    return ws + [" ".join(w.strip() for w in ws), "the " + ws[0].strip() + " " + ws[1].strip()]


@pytest.fixture(scope="module")
def handles():
    """one handle per layout for the whole module: every batch of it takes a census, whatever the table has become meanwhile"""
    tokenizers = pytest.importorskip("tokenizers")
    import tokenizers_amd as ta
    out = {}
    for layout in ("gpt2", "bert"):
        js = _json_of(layout)
        tok = ta.Tokenizer.from_str(js, device=0)
        out[layout] = (js, tok, tokenizers.Tokenizer.from_str(js), tok.hot_table(words=True)["eligible_ids"])
    return out


@pytest.mark.parametrize("text", sorted(TEXTS))
@pytest.mark.parametrize("layout", ["gpt2", "bert"])
def test_census_equals_a_python_recount(layout, text, handles):
    js, tok, ref, eligible = handles[layout]
    docs = TEXTS[text] or _words_12_13(js, eligible)
    want, total = R.recount(ref, js, docs, eligible)
    before = tok.info
    tok.encode_batch_csr(docs)
    after = tok.info
    if total == 0:               # nothing to sample: the counts stay what the last census left
        assert after["hot_generation"] == before["hot_generation"]
        return
    assert after["hot_census_sample"] == total
    assert tok.hot_census_counts() == want
    if text == "more_than_64_tiles":
        n_tiles = -(-sum(len(d.encode()) for d in docs) // TILE)
        assert n_tiles > 64 and len(set(R.sample_tiles(n_tiles * TILE))) == 64
    if text == "words_of_12_and_13_bytes":
        lens = [len(R.token_bytes(js)[i]) for i in want]
        assert 12 in lens and max(lens) == 12, lens


@pytest.mark.parametrize("name", ["bytelevel_prefix_trim_3000", "bert_wordpiece_4000", "llama3_small_6000", "wordlevel_whitespace_c1"])
def test_golden_vectors_before_the_census_on_it_and_after_the_rebuild(name):
    import tokenizers_amd as ta
    js, v = load_tokenizer_json(name), load_vectors(name)

    def check(tok):
        got = tok.encode_batch(v["docs"], add_special_tokens=False)
        for i, doc in enumerate(v["docs"]):
            assert got[i].ids == v["ids"][i], doc
            assert [list(x) for x in got[i].offsets] == v["offsets_char"][i], doc
            assert got[i].word_ids == v["words"][i], doc

    tok = ta.Tokenizer.from_str(js, device=0)
    tok.hot_adapt(False)
    check(tok)                                   # the load-time table, no census
    assert tok.info["hot_census_sample"] == 0
    tok.hot_adapt(True)
    check(tok)                                   # the batch that takes the census
    first = tok.info
    assert first["hot_census_sample"] > 0 and first["hot_generation"] == 1, first      # (the vectors' text is nothing like id order)
    assert first["hot_rate_selected"] >= first["hot_rate_in_use"] + 0.02
    check(tok)                                   # the rebuilt table; its census finds nothing to gain
    second = tok.info
    assert second["hot_generation"] == 1 and second["hot_rate_in_use"] == first["hot_rate_selected"], second
    ids_only = tok.encode_batch_csr(v["docs"])
    assert [list(ids_only.ids[ids_only.tok_offsets[i]:ids_only.tok_offsets[i + 1]]) for i in range(len(v["docs"]))] == v["ids"]


# ---- the launch log of a census batch ----
DOCS = ["The quick brown fox jumps over the lazy dog.", "", "café naïve 中文 Жук \U0001F600 ok", "hello hello hello world world", "It's 2024, isn't it? Yes!!"]
SEQ_CASES = {"gpt2_ids": ("gpt2", {}), "gpt2_char_offsets_words": ("gpt2", dict(offsets="char", word_ids=True)), "bert_ids": ("bert", {})}


def launch_sequence(case) -> list[str]:
    """the log of three calls on a fresh handle: the census batch (and the rebuild behind its synchronisation), the batch after it (a
    census again at period 1, nothing to gain), and one with the adaptation switched off"""
    import tokenizers_amd as ta
    layout, kw = SEQ_CASES[case]
    tok = ta.Tokenizer.from_str(_json_of(layout), device=0)
    lib = _lib.load()
    lib.simt_launch_log_read.restype = C.c_size_t
    lib.simt_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
    lib.simt_launch_log_clear()
    tok.encode_batch_csr(DOCS, **kw)
    tok.encode_batch_csr(DOCS, **kw)
    tok.hot_adapt(False)
    tok.encode_batch_csr(DOCS, **kw)
    n = lib.simt_launch_log_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.simt_launch_log_read(buf, n)
    assert tok.info["hot_generation"] == 1
    return buf.raw[:n].decode().splitlines()


@pytest.mark.parametrize("case", sorted(SEQ_CASES))
def test_launch_sequence_of_a_census_batch_is_the_recorded_one(case):
    with open(FIXTURE, encoding="utf-8") as fh:
        want = json.load(fh)["cases"][case]
    got = launch_sequence(case)
    first = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, "first difference at call %d: got %r, recorded %r" % (first, got[first:first + 3], want[first:first + 3])
    census = [l for l in got if "k_hot_census" in l]
    assert len(census) == 2, census              # (two censuses, none with the adaptation off)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_hot_census_simt.py --record"
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    os.environ.update(HOOKS)
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_hot_census_simt.py (its --record): a census batch with the rebuild behind its "
                     "synchronisation, the next batch, and one with the adaptation off; record it again only for a change that moves a launch on purpose",
           "cases": {c: launch_sequence(c) for c in sorted(SEQ_CASES)}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
