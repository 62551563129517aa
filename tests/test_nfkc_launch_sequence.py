"""What the host code enqueues for a batch behind the NFKC normalizer (NORM_NFKC) in front of the U+2581 front, call by call, compared with
the recorded sequences of tests/golden/launch_sequences_nfkc.json -- the new configurations' own fixture, written by
`python tests/test_nfkc_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of the SIMT
emulation).  The sequences of every other configuration stay in their own fixtures, untouched."""
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

FIXTURE = os.path.join(GOLD, "launch_sequences_nfkc.json")
BPE, UNI = "nfkc_spm_bpe", "nfkc_unigram"
IN_TEXT = base.DOCS + ["a<raw>\u0301 \uff23af\u00e9 au lait", "<raw>", "xCaf\u00e9x <raw> y"]
CASES = [
    base._case("bpe_ids", BPE),
    base._case("bpe_char_offsets_words", BPE, offsets="char", word_ids=True),
    base._case("bpe_special_tokens_pairs", BPE, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("bpe_trunc_overflow", BPE, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("bpe_added_speculated", BPE, inputs=IN_TEXT, offsets="char"),
    base._case("bpe_added_no_speculation", BPE, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
    base._case("unigram_ids", UNI),
    base._case("unigram_byte_offsets", UNI, offsets="byte"),
    base._case("unigram_added_no_speculation", UNI, inputs=IN_TEXT, offsets="byte", no_speculation=True),
    base._case("bpe_all_empty", BPE, inputs=["", ""]),
]
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


def _count(log, kernel):
    return sum(kernel in l for l in log)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_launch_sequence_is_the_recorded_one(name, recorded):
    got, want = base.launch_sequence(BY_NAME[name]), recorded[name]
    first = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, "first difference at call %d: got %r, recorded %r" % (first, got[first:first + 3], want[first:first + 3])
    runs = 2 if name == "bpe_added_speculated" else 1                  # (the speculating batch saw an added token and is run again)
    if name == "bpe_all_empty":
        assert _count(got, "k_nfkc_") == 0 and _count(got, "k_nfc_") == 0
        return
    # every batch takes the K mode's own kernels, once per run, with the length backstop between them: no quick check, none of NFC's
    # or the Precompiled normalizer's count / write kernels
    assert _count(got, "k_nfkc_count") == runs and _count(got, "k_nfkc_write") == runs and _count(got, "k_pc_check_len") == runs
    assert _count(got, "k_nfc_count") == 0 and _count(got, "k_nfc_write") == 0 and _count(got, "k_nfc_check") == 0
    assert _count(got, "k_pc_count") == 0 and _count(got, "k_pc_write") == 0 and _count(got, "k_bn_count") == 0


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_nfkc_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_nfkc_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of these configurations on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
