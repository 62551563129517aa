"""What the host code enqueues for a batch behind a chain of NFD / Lowercase / StripAccents (NORM_CHAIN), call by call, compared with the
recorded sequences of tests/golden/launch_sequences_unicode_chain.json -- the new configurations' own fixture, written by
`python tests/test_unicode_chain_launch_sequence.py --record` the way tests/test_launch_sequence.py writes its own (the launch log of the
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

FIXTURE = os.path.join(GOLD, "launch_sequences_unicode_chain.json")
NLS, LWL, SLB, NL = "chain_nls_wp", "chain_l_wl", "chain_sl_bpe", "chain_nl_wp"
IN_TEXT = base.DOCS + ["a<raw>\u0301 CAF\u00c9 au lait", "<raw>", "xCaf\u00c9x <raw> y"]
# context free per char: the BertNormalizer's kernels over the chain's tables
FREE = [
    base._case("nls_wordpiece", NLS),
    base._case("nls_wordpiece_char_offsets_words", NLS, offsets="char", word_ids=True),
    base._case("nls_wordpiece_special_tokens_pairs", NLS, inputs=base.PAIRS, add_special_tokens=True, offsets="char", word_ids=True),
    base._case("nls_wordpiece_trunc_overflow", NLS, edit=base._with(truncation=base.TRUNC), add_special_tokens=True, overflowing=True),
    base._case("l_wordlevel_byte_offsets", LWL, offsets="byte"),
    base._case("sl_bpe_added_speculated", SLB, inputs=IN_TEXT, offsets="char"),
    base._case("sl_bpe_added_no_speculation", SLB, inputs=IN_TEXT, offsets="char", word_ids=True, no_speculation=True),
]
# NFD stays in the text: the NFC normalizer's kernels in their NFD mode
VISIBLE = [
    base._case("nl_wordpiece", NL),
    base._case("nl_wordpiece_char_offsets_words", NL, offsets="char", word_ids=True),
    base._case("nl_wordpiece_added_no_speculation", NL, inputs=IN_TEXT, offsets="byte", no_speculation=True),
]
CASES = FREE + VISIBLE + [base._case("nls_all_empty", NLS, inputs=["", ""])]
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
    runs = 2 if name == "sl_bpe_added_speculated" else 1               # (the speculating batch saw an added token and is run again)
    if BY_NAME[name] in FREE:
        # count and write once per run, nothing that looks across chars, nothing of the NFC normalizer
        assert _count(got, "k_bn_count") == runs and _count(got, "k_bn_write") == runs
        assert _count(got, "k_bn_reorder_fix") == 0 and _count(got, "k_nfc_") == 0
    elif BY_NAME[name] in VISIBLE:
        # every batch takes the normalizer's general path: no quick check, no speculation on it
        assert _count(got, "k_nfc_count") == 1 and _count(got, "k_nfc_write") == 1
        assert _count(got, "k_nfc_check") == 0 and _count(got, "k_bn_count") == 0 and _count(got, "k_bn_reorder_fix") == 0
    else:
        assert _count(got, "k_bn_") == 0 and _count(got, "k_nfc_") == 0


if __name__ == "__main__":
    from tokenizers_amd import _lib
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_unicode_chain_launch_sequence.py --record"
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_unicode_chain_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of these configurations on purpose",
           "cases": {c["name"]: base.launch_sequence(c) for c in CASES}}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: len(v) for k, v in out["cases"].items()})
