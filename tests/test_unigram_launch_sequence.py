"""What the host code enqueues for a batch of a Unigram model behind the "▁" front (MODEL_UNIGRAM), call by call, compared with the
recorded sequences of tests/golden/launch_sequences_unigram.json -- the new configuration's own fixture, written by
`python tests/test_unigram_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of the
SIMT emulation).  The sequences of every other configuration stay in tests/golden/launch_sequences.json, untouched."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_launch_sequence as base
from tests.helpers import GOLD

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

FIXTURE = os.path.join(GOLD, "launch_sequences_unigram.json")
UNI, ADV = "unigram_ms", "unigram_adv"
IN_TEXT = base.DOCS + ["a<s>b c</s> 中ꙮ", "<s>"]
CASES = [
    base._case("unigram", UNI),
    base._case("unigram_byte_offsets", UNI, offsets="byte"),
    base._case("unigram_char_offsets_words", UNI, offsets="char", word_ids=True),
    base._case("unigram_no_byte_fallback_char_offsets", ADV, offsets="char", word_ids=True),
    base._case("unigram_added_speculated", UNI, inputs=IN_TEXT, offsets="char"),
    base._case("unigram_added_no_speculation", UNI, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
    base._case("unigram_special_tokens", UNI, add_special_tokens=True),
    base._case("unigram_pretokenized", UNI, inputs=[w for w in base.WORDS if w], is_pretokenized=True, offsets="char", word_ids=True),
    base._case("unigram_pairs", UNI, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("unigram_trunc_overflow", UNI, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("unigram_all_empty", UNI, inputs=["", ""]),
]
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_launch_sequence_is_the_recorded_one(name, recorded):
    got, want = base.launch_sequence(BY_NAME[name]), recorded[name]
    first = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, "first difference at call %d: got %r, recorded %r" % (first, got[first:first + 3], want[first:first + 3])
    if name != "unigram_all_empty":
        # ONE model launch behind the lookup, no merge kernel; the run-offsets pair only with offsets AND byte_fallback
        runs = 2 if name == "unigram_added_speculated" else 1              # (the speculating batch saw an added token and is run again)
        assert sum("k_unigram_all" in l for l in got) == runs and not any("k_bpe_merge" in l or "k_wordpiece" in l for l in got)
        want_runs = name in ("unigram_byte_offsets", "unigram_char_offsets_words", "unigram_added_speculated", "unigram_added_no_speculation", "unigram_pretokenized", "unigram_pairs")
        assert any("k_unigram_run_offsets" in l for l in got) == want_runs


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_unigram_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_unigram_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of this configuration on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
