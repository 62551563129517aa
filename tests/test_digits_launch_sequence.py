"""What the host code enqueues for a batch behind Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family (PT_DIGITS_GPT2),
call by call, compared with the recorded sequences of tests/golden/launch_sequences_digits.json -- the new configuration's own fixture,
written by `python tests/test_digits_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of
the SIMT emulation).  The sequences of every other configuration stay in their own fixtures, untouched."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import digits_cases as dc
from tests import test_launch_sequence as base
from tests.helpers import GOLD

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

FIXTURE = os.path.join(GOLD, "launch_sequences_digits.json")
IND, CON = dc.NAMES
IN_TEXT = base.DOCS + [dc.USER + "Hello 123 x=4" + dc.ASSISTANT + "  ok 5" + dc.EOS]
CASES = [
    base._case("digits", IND),
    base._case("digits_contiguous", CON),
    base._case("digits_byte_offsets", IND, offsets="byte"),
    base._case("digits_char_offsets_words", IND, offsets="char", word_ids=True),
    base._case("digits_contiguous_char_offsets", CON, offsets="char"),
    base._case("digits_added_speculated", IND, inputs=IN_TEXT, offsets="char"),
    base._case("digits_added_no_speculation", IND, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
    base._case("digits_special_tokens", IND, add_special_tokens=True),
    base._case("digits_pretokenized", IND, inputs=[w for w in base.WORDS if w], is_pretokenized=True, offsets="char", word_ids=True),
    base._case("digits_pairs", IND, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("digits_trunc_overflow", IND, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("digits_nfc_in_front", IND, edit=base._with(normalizer={"type": "NFC"}), offsets="char"),
    base._case("digits_all_empty", IND, inputs=["", ""]),
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
    if name != "digits_all_empty":
        mode = "false" if "contiguous" in name else "true"
        other = "true" if mode == "false" else "false"
        assert any("k_pretok_digits<" + mode in l for l in got) and not any("k_pretok_digits<" + other in l for l in got), [l for l in got if "pretok" in l]
        assert not any("k_pretok_gpt2_seq" in l or "k_pretok_llama3" in l for l in got)


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_digits_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_digits_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of this configuration on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
