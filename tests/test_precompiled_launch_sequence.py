"""What the host code enqueues for a batch of a Unigram model behind the Precompiled normalizer (NORM_PRECOMPILED: the XLM-R layout and
Precompiled in front of bare Metaspace), call by call, compared with the recorded sequences of
tests/golden/launch_sequences_precompiled.json -- the new configurations' own fixture, written by
`python tests/test_precompiled_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of the
SIMT emulation).  The sequences of every other configuration stay in their own fixtures, untouched."""
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

FIXTURE = os.path.join(GOLD, "launch_sequences_precompiled.json")
XLMR, PMS = "precompiled_xlmr", "precompiled_ms"
IN_TEXT = base.DOCS + ["a<s>b c</s> \u4e2d\ufb03", "<mask>", "\ufeffx <mask> y"]
CASES = [
    base._case("xlmr", XLMR),
    base._case("xlmr_byte_offsets", XLMR, offsets="byte"),
    base._case("xlmr_char_offsets_words", XLMR, offsets="char", word_ids=True),
    base._case("ms_char_offsets_words", PMS, offsets="char", word_ids=True),
    base._case("xlmr_added_speculated", XLMR, inputs=IN_TEXT, offsets="char"),
    base._case("xlmr_added_no_speculation", XLMR, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
    base._case("ms_added_no_speculation", PMS, inputs=IN_TEXT, no_speculation=True),
    base._case("xlmr_special_tokens", XLMR, add_special_tokens=True),
    base._case("xlmr_pairs", XLMR, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("xlmr_trunc_overflow", XLMR, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("xlmr_all_empty", XLMR, inputs=["", ""]),
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
    if name != "xlmr_all_empty":
        # the normalizer's count and write once per run, in front of the front's; the lost chars' fix only with offsets
        runs = 2 if name == "xlmr_added_speculated" else 1                 # (the speculating batch saw an added token and is run again)
        assert sum("k_pc_count" in l for l in got) == runs and sum("k_pc_write" in l for l in got) == runs
        assert sum("k_ms_count" in l for l in got) == runs and sum("k_unigram_all" in l for l in got) == runs
        assert next(k for k, l in enumerate(got) if "k_pc_write" in l) < next(k for k, l in enumerate(got) if "k_ms_count" in l)
        with_offsets = "offsets" in name or name in ("xlmr_added_speculated", "xlmr_added_no_speculation", "xlmr_pairs")
        assert any("k_pc_lost_fix" in l for l in got) == with_offsets
        assert any("k_pc_translate_matches" in l for l in got) == ("added" in name)


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_precompiled_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_precompiled_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of these configurations on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
