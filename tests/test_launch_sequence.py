"""What the host code enqueues for a batch, call by call: every kernel launch with its grid and block, every asynchronous memset /
memcpy with its byte count and every stream synchronisation, for one small batch per configuration of the batch pipeline
(capi/pipeline.cpp, capi/epilogue.cpp), compared with the recorded sequences of tests/golden/launch_sequences.json.

The sequences come from the launch log of the SIMT emulation (tests/harness/simt/hip/hip_runtime.h: simt_launch_log_clear /
simt_launch_log_read), which compiles csrc/ unchanged and runs the real host code.  The fixture is a RECORDED RESULT: it was written by
`python tests/test_launch_sequence.py --record` from the csrc/ of the commit BEFORE run_pipeline was split into stages, and was not
regenerated afterwards -- the split had to reproduce it.  A change that moves a launch on purpose records the fixture again, and its
diff then shows exactly what moved."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tokenizers_amd import _lib

from tests.harness import simt_build
from tests.helpers import GOLD, load_tokenizer_json

FIXTURE = os.path.join(GOLD, "launch_sequences.json")

# a dozen short documents: an empty one, non-ASCII ones, pre-tokens of 17-32, 33-64 and more than 64 bytes
DOCS = ["The quick brown fox jumps over the lazy dog.", "", "café naïve 中文 Жук \U0001F600 ok",
        "some counterrevolutionaries here", "supercalifragilisticexpialidociousnesses", "b" + "ab" * 35 + " end",
        "It's 2024, isn't it? Yes!!", "  leading and trailing  ", "tabs\tand\nnewlines\r\n", "hello hello hello world world", "A",
        "MixedCase camelCaseWord HTTPServer's"]
WORDS = [d.split() for d in DOCS]
PAIRS = [(DOCS[i], DOCS[i + 1]) for i in range(0, len(DOCS), 2)]
MIXED = [DOCS[0], (DOCS[2], DOCS[3]), DOCS[1], (DOCS[4], DOCS[6]), DOCS[5], (DOCS[1], DOCS[9])]
# (a queue of 1 / 100000 of the text holds 64 entries a sub-queue: a few hundred distinct unknown words overflow it once)
MANY = [" ".join("q%dz%dx" % (i, 7 * i + j) for j in range(12)) for i in range(40)]

TRUNC = {"direction": "Right", "max_length": 10, "strategy": "LongestFirst", "stride": 2}
LONGEST = {"strategy": "BatchLongest", "direction": "Right", "pad_to_multiple_of": 4, "pad_id": 0, "pad_type_id": 0, "pad_token": "[PAD]"}
FIXED = {"strategy": {"Fixed": 24}, "direction": "Left", "pad_to_multiple_of": None, "pad_id": 0, "pad_type_id": 0, "pad_token": "[PAD]"}
HOOKS = {"TKAMD_TEST_HOOKS": "1"}


def _lean(d):
    d["pre_tokenizer"]["add_prefix_space"] = False
    d["post_processor"] = None


def _noregex(d):
    _lean(d)
    d["pre_tokenizer"]["use_regex"] = False


def _with(**sections):
    def edit(d):
        d.update(sections)
    return edit


def _case(name, tokenizer, inputs=DOCS, edit=None, env=None, word_cache=False, calls=1, **kw):
    return dict(name=name, tokenizer=tokenizer, inputs=inputs, edit=edit, env=env or {}, word_cache=word_cache, calls=calls, kw=kw)


BERT = "bert_wordpiece_4000_specials"
L3S = "llama3_small_6000_specials"
CASES = [
    # the lean ByteLevel path: ids only, byte offsets, char offsets + word ids (the lead mask rides in the pre-tokenizer)
    _case("lean_ids", "bytelevel_prefix_trim_3000", edit=_lean),
    _case("lean_byte_offsets", "bytelevel_prefix_trim_3000", edit=_lean, offsets="byte"),
    _case("lean_char_offsets_words", "bytelevel_prefix_trim_3000", edit=_lean, offsets="char", word_ids=True),
    _case("lean_noregex", "bytelevel_prefix_trim_3000", edit=_noregex),
    _case("prefix_space_offsets", "bytelevel_prefix_trim_3000", offsets="char"),
    # Llama-3 Split: plain, and with special tokens in the text -- speculated (detect pass, the batch again) and matched outright
    _case("llama3", "llama3_small_6000"),
    _case("llama3_char_offsets", "llama3_small_6000", offsets="char", word_ids=True),
    _case("llama3_specials_speculated", L3S, inputs=DOCS + ["<|begin_of_text|>hello<|end_of_text|> world"], offsets="char"),
    _case("added_tokens_plain_text", "bert_wordpiece_4000_added"),
    _case("llama3_specials_no_speculation", L3S, inputs=DOCS + ["<|begin_of_text|>hello<|end_of_text|> world"], offsets="char",
          no_speculation=True),
    _case("split_o200k", "split_o200k", offsets="char"),
    _case("bert_char_offsets", "bert_wordpiece_4000", offsets="char", word_ids=True),
    _case("bert_added_in_text", "bert_wordpiece_4000_added", inputs=DOCS + ["a NewWord and [MASK] in café wide", "[CLS]NewWord"],
          offsets="char", word_ids=True, no_speculation=True),
    _case("bert_added_speculated", "bert_wordpiece_4000_added", inputs=DOCS + ["a NewWord and [MASK] in café wide"]),
    _case("prefix_space_added", "bytelevel_prefix_trim_3000", inputs=DOCS + ["say <new1> twice<new1>"], offsets="char",
          edit=_with(added_tokens=[{"id": 3000, "content": "<new1>", "single_word": False, "lstrip": False, "rstrip": False,
                                    "normalized": False, "special": True}]), no_speculation=True),
    _case("wordlevel", "wordlevel_whitespace_c1", offsets="byte"),
    _case("bpe_chars_no_unk_offsets", "bpe_ws_no_unk", offsets="char", word_ids=True),
    _case("bpe_chars_ignore_merges", "bpe_ws_ignore_merges"),
    _case("bpe_chars_ignore_merges_no_unk_offsets", "bpe_ws_ignore_merges_no_unk", offsets="byte"),
    _case("spm_llama2", "spm_bpe_llama2", add_special_tokens=True),
    _case("spm_llama2_added_in_text", "spm_bpe_llama2", inputs=DOCS + ["a<s>b </s>"], offsets="char", no_speculation=True),
    _case("spm_split_words", "spm_bpe_split", offsets="char", word_ids=True),
    _case("spm_llama2_words", "spm_bpe_llama2", offsets="byte", word_ids=True),
    # inputs: lists of words, pairs, both kinds mixed
    _case("pretokenized", BERT, inputs=[w for w in WORDS if w] + [[]], is_pretokenized=True, offsets="char", word_ids=True, add_special_tokens=True),
    _case("pretokenized_trim", "bytelevel_prefix_trim_3000", inputs=[w for w in WORDS if w], is_pretokenized=True, offsets="char", word_ids=True),
    _case("pairs", BERT, inputs=PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    _case("mixed", BERT, inputs=MIXED, mixed=True, add_special_tokens=True),
    # the epilogues
    _case("add_special_alone", BERT, edit=_with(post_processor={"type": "TemplateProcessing", "single": [
        {"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}}],
        "pair": [{"Sequence": {"id": "A", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 0}}],
        "special_tokens": {"[CLS]": {"id": "[CLS]", "ids": [2], "tokens": ["[CLS]"]}, "[SEP]": {"id": "[SEP]", "ids": [3], "tokens": ["[SEP]"]}}}),
        add_special_tokens=True, offsets="byte"),
    _case("typed_single", BERT, add_special_tokens=True),
    _case("trunc_longest", BERT, edit=_with(truncation=TRUNC, padding=LONGEST), add_special_tokens=True, offsets="char", word_ids=True),
    _case("trunc_longest_overflow", BERT, edit=_with(truncation=TRUNC, padding=LONGEST), add_special_tokens=True, offsets="char", overflowing=True),
    _case("trunc_overflow_no_padding", BERT, edit=_with(truncation=TRUNC), overflowing=True),
    _case("trunc_longest_pairs", BERT, inputs=PAIRS, edit=_with(truncation=TRUNC, padding=LONGEST), add_special_tokens=True),
    _case("trunc_longest_pairs_overflow", BERT, inputs=PAIRS, edit=_with(truncation=TRUNC, padding=LONGEST), add_special_tokens=True, offsets="byte",
          overflowing=True),
    _case("trunc_mixed_overflow", BERT, inputs=MIXED, mixed=True, edit=_with(truncation=TRUNC), overflowing=True),
    _case("fixed_padding", BERT, edit=_with(padding=FIXED), add_special_tokens=True),
    _case("fixed_padding_pairs", BERT, inputs=PAIRS, edit=_with(padding=FIXED)),
    _case("trim1_truncation", "bytelevel_prefix_trim_3000", edit=_with(truncation=TRUNC), offsets="char"),
    _case("all_empty", BERT, inputs=["", "", ""], add_special_tokens=True, offsets="char", word_ids=True),
    _case("all_empty_pairs", BERT, inputs=[("", ""), ("", "")], edit=_with(padding=LONGEST), add_special_tokens=True),
    _case("all_empty_plain", "wordlevel_whitespace_c1", inputs=["", ""]),
    # the work queue overflows once: run again from the synchronisation, and from the overflow epilogue's read-back
    _case("queue_overflow", "bytelevel_prefix_trim_3000", inputs=MANY, env={"TKAMD_Q16_DIV": "100000", **HOOKS}),
    _case("queue_overflow_in_epilogue", "bytelevel_prefix_trim_3000", inputs=MANY, edit=_with(truncation=TRUNC), overflowing=True,
          env={"TKAMD_Q16_DIV": "100000", **HOOKS}),
    _case("queue_overflow_in_pair_epilogue", BERT, inputs=list(zip(MANY[::2], MANY[1::2])), edit=_with(truncation=TRUNC), overflowing=True,
          env={"TKAMD_Q16_DIV": "100000", **HOOKS}),
    # test hooks of the model stage
    _case("claims_off", "bytelevel_prefix_trim_3000", edit=_lean, offsets="byte", env={"TKAMD_CLAIMS": "0", **HOOKS}),
    _case("claims_off_wordpiece", "bert_wordpiece_4000", env={"TKAMD_CLAIMS": "0", **HOOKS}),
    _case("merge_two", "bytelevel_prefix_trim_3000", edit=_lean, env={"TKAMD_MERGE_TWO": "1", **HOOKS}),
    _case("merge_pair_off", "bytelevel_prefix_trim_3000", edit=_lean, env={"TKAMD_MERGE_PAIR": "0", **HOOKS}),
    _case("force_lane_merge", "bytelevel_prefix_trim_3000", edit=_lean, env={"TKAMD_FORCE_LANE_MERGE": "1", **HOOKS}),
    _case("phases", "bytelevel_prefix_trim_3000", edit=_lean, env={"TKAMD_PHASES": "1", **HOOKS}),
    _case("poison_ntext", "bert_wordpiece_4000", offsets="char", env={"TKAMD_POISON_NTEXT": "1", **HOOKS}),
    _case("word_cache", "bytelevel_prefix_trim_3000", edit=_lean, word_cache=True, calls=2),
    _case("word_cache_wordpiece", "bert_wordpiece_4000", word_cache=True, calls=2),
    _case("word_cache_with_offsets", "bytelevel_prefix_trim_3000", edit=_lean, word_cache=True, offsets="byte"),
    _case("second_batch_same_handle", "bert_wordpiece_4000_added", calls=2, offsets="char"),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@pytest.fixture(scope="module", autouse=True)
def simt_library():
    """ctypes opens the host build for the tests of this module (like tests/test_simt_pipeline.py)"""
    simt_build.build()
    saved = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    try:
        yield
    finally:
        _lib.LIB_PATH, _lib._lib = saved


def launch_sequence(case) -> list[str]:
    """the log of the case's encode calls on a fresh handle; a case that sets test hooks runs in a process of its own (some hooks are read
    once per process, and a batch whose queue overflowed reads rows nobody wrote: fresh memory makes that the same every time)"""
    if case["env"] and os.environ.get("TKAMD_TEST_HOOKS") != "1":
        import subprocess
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case["name"]], env=dict(os.environ, **case["env"]),
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads(r.stdout.splitlines()[-1])
    import tokenizers_amd as ta
    saved = {k: os.environ.get(k) for k in list(case["env"]) + ["TKAMD_PACED"]}
    os.environ.update(case["env"], TKAMD_PACED="0")         # (the packed entry: one call, no helper threads)
    try:
        d = json.loads(load_tokenizer_json(case["tokenizer"]))
        if case["edit"]:
            case["edit"](d)
        tok = ta.Tokenizer.from_str(json.dumps(d), device=0)
        if case["word_cache"]:
            tok.word_cache(True)
        lib = _lib.load()
        lib.simt_launch_log_read.restype = C.c_size_t
        lib.simt_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        lib.simt_launch_log_clear()
        kw = dict(case["kw"])
        if kw.pop("no_speculation", False):                # TKAMD_NO_SPECULATION: the added tokens' matching passes outright
            flags_of = tok._flags
            tok._flags = lambda *a: flags_of(*a) | _lib.NO_SPECULATION
        for _ in range(case["calls"]):
            if kw.get("mixed"):
                is_pair = lambda it: isinstance(it, (tuple, list))
                tok._encode_mixed(case["inputs"], kw.get("offsets", "none"), kw.get("word_ids", False), kw.get("add_special_tokens", False), False,
                                  kw.get("overflowing", False), is_pair)
            else:
                tok.encode_batch_csr(case["inputs"], **kw)
        n = lib.simt_launch_log_read(None, 0)
        buf = C.create_string_buffer(n + 1)
        lib.simt_launch_log_read(buf, n)
        if "TKAMD_Q16_DIV" in case["env"]:
            assert tok.queue_sizes()["q16_div"] == 2, "the queue did not overflow exactly once"
        return buf.raw[:n].decode().splitlines()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_launch_sequence_is_the_recorded_one(name, recorded):
    """the calls the host enqueues for this configuration, in order, equal the sequence recorded before run_pipeline was split
    (tests/golden/launch_sequences.json: a recorded result, not regenerated by the split)"""
    got, want = launch_sequence(BY_NAME[name]), recorded[name]
    first = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, "first difference at call %d: got %r, recorded %r" % (first, got[first:first + 3], want[first:first + 3])
    assert any(l.startswith("launch ") for l in got)


if __name__ == "__main__":
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    if sys.argv[1:2] == ["--case"]:
        print(json.dumps(launch_sequence(BY_NAME[sys.argv[2]])))
        sys.exit(0)
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_launch_sequence.py, written by its --record from the csrc/ of the commit "
                     "before run_pipeline was split into stages; record it again only for a change that moves a launch on purpose",
           "cases": {c["name"]: launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
