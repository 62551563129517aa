"""What the host code enqueues for a batch behind BLOOM's Split + ByteLevel(use_regex=false) (PT_BLOOM), call by call, compared with the
recorded sequences of tests/golden/launch_sequences_bloom.json -- the new configuration's own fixture, written by
`python tests/test_bloom_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of the SIMT
emulation).  The sequences of every other configuration stay in their own fixtures, untouched."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bloom_cases as bc
from tests import test_launch_sequence as base
from tests.helpers import GOLD

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

FIXTURE = os.path.join(GOLD, "launch_sequences_bloom.json")
IN_TEXT = base.DOCS + [bc.USER + "Hello, world. x " + bc.ASSISTANT + "  ok (fine) " + bc.EOS]
CASES = [
    base._case("bloom", bc.NAME),
    base._case("bloom_byte_offsets", bc.NAME, offsets="byte"),
    base._case("bloom_char_offsets_words", bc.NAME, offsets="char", word_ids=True),
    base._case("bloom_added_speculated", bc.NAME, inputs=IN_TEXT, offsets="char"),
    base._case("bloom_added_no_speculation", bc.NAME, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
    base._case("bloom_special_tokens", bc.NAME, add_special_tokens=True),
    base._case("bloom_pretokenized", bc.NAME, inputs=[w for w in base.WORDS if w], is_pretokenized=True, offsets="char", word_ids=True),
    base._case("bloom_pairs", bc.NAME, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("bloom_trunc_overflow", bc.NAME, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("bloom_no_added_tokens", bc.NAME, edit=base._with(added_tokens=[])),      # (what the lean path asks of a file, but for the kind)
    base._case("bloom_all_empty", bc.NAME, inputs=["", ""]),
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
    if name != "bloom_all_empty":
        assert any("k_pretok_bloom<" in l for l in got), [l for l in got if "pretok" in l]
        if name in ("bloom", "bloom_char_offsets_words"):       # (the lead-byte mask rides along for char offsets)
            lead = "true" if "char" in name else "false"
            assert all("k_pretok_bloom<" + lead in l for l in got if "k_pretok_bloom" in l)
        # the general order (the lean path has no k_sanitize_csr), and no other pre-tokenizer's kernel
        assert any("k_sanitize_csr" in l for l in got)
        assert not any("k_pretok_gpt2_seq" in l or "k_pretok_llama3" in l or "k_pretok_digits" in l for l in got)


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_bloom_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_bloom_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of this configuration on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
