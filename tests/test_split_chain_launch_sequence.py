"""What the host code enqueues for a batch behind the chained Split pre-tokenizer of DeepSeek-V3 / R1 (PT_SPLIT_CHAIN), call by call,
compared with the recorded sequences of tests/golden/launch_sequences_split_chain.json -- the new configuration's own fixture, written by
`python tests/test_split_chain_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of the
SIMT emulation).  The sequences of every other configuration stay in tests/golden/launch_sequences.json, untouched."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import split_chain_cases as sc
from tests import test_launch_sequence as base
from tests.helpers import GOLD

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

FIXTURE = os.path.join(GOLD, "launch_sequences_split_chain.json")
DS3 = "ds3_chain"
IN_TEXT = base.DOCS + [sc.USER + "Hello 123 中文" + sc.ASSISTANT + "  ok" + sc.EOS]
CASES = [
    base._case("ds3", DS3),
    base._case("ds3_byte_offsets", DS3, offsets="byte"),
    base._case("ds3_char_offsets_words", DS3, offsets="char", word_ids=True),
    base._case("ds3_added_speculated", DS3, inputs=IN_TEXT, offsets="char"),
    base._case("ds3_added_no_speculation", DS3, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
    base._case("ds3_special_tokens", DS3, add_special_tokens=True),
    base._case("ds3_pretokenized", DS3, inputs=[w for w in base.WORDS if w], is_pretokenized=True, offsets="char", word_ids=True),
    base._case("ds3_pairs", DS3, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("ds3_trunc_overflow", DS3, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("ds3_nfc_in_front", DS3, edit=base._with(normalizer={"type": "NFC"}), offsets="char"),
    base._case("ds3_all_empty", DS3, inputs=["", ""]),
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
    if name != "ds3_all_empty":
        assert any("k_pretok_ds3_lane" in l for l in got) and any("k_pretok_ds3_slow" in l for l in got)
        assert not any("k_pretok_llama3" in l for l in got)


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_split_chain_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_split_chain_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of this configuration on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
