"""The seeded cross-layout differential on the device: every family's cases 0..11 of tests/fuzz_cases.py -- the fixture with another
post-processor, random added tokens, truncation / padding, the options of its components flipped; single, pair, pre-tokenized and mixed
input -- against what the 0.22.2 wheel answered (tests/golden/fuzz_layouts_vectors.json.gz, tools/make_golden_fuzz.py): every field of
every encoding and overflowing encoding, an error where the wheel raised one, the pinned message where this library refuses, and
decode_batch of the encoded and of shuffled ids wherever the decoder is on the path.  It needs no wheel.  The `found` tests are the
reduced cases of what the differential found; each fails without its fix."""
import pytest

import tokenizers_amd as ta
from tests import fuzz_cases as fc
from tests.fuzz_cases import vectors

pytestmark = pytest.mark.gpu


def hold_case(case, rec, what):
    """one case on the device against its record; returns 'refused' / 'raised' / 'compared'"""
    assert fc.digest(case) == rec["digest"], what
    try:
        tok = ta.Tokenizer.from_str(case["json"], device=0)
    except ta.UnsupportedError as e:
        assert rec["refused"] is not None, (what, "refused at load, the vectors say it loads", str(e))
        assert str(e)[:fc.REFUSAL_CHARS] == rec["refused"], what
        return "refused"
    kw = dict(add_special_tokens=case["add_special_tokens"], is_pretokenized=case["is_pretokenized"])
    tok.encode_special_tokens = case["encode_special_tokens"]
    if rec["refused"] is not None:
        # a refusal at the call (a template the single path does not take, ...): the message is pinned like a load's
        assert rec["refused"].startswith("encode: "), (what, "loads, the vectors say it is refused", rec["refused"])
        with pytest.raises(ta.UnsupportedError) as ei:
            tok.encode_batch(fc.call_inputs(case), **kw)
        assert ("encode: " + str(ei.value))[:fc.REFUSAL_CHARS] == rec["refused"], what
        return "refused"
    if rec["raised"]:
        with pytest.raises((ValueError, ta.TokenizersAmdError)) as ei:
            tok.encode_batch(fc.call_inputs(case), **kw)
        assert not isinstance(ei.value, ta.UnsupportedError), (what, str(ei.value))
        return "raised"
    got = tok.encode_batch(fc.call_inputs(case), **kw)
    assert len(got) == len(rec["enc"]), what
    for i, (e, exp) in enumerate(zip(got, rec["enc"])):
        have = fc.deep(e)
        assert len(have) == len(exp), (what, i, "overflowing encodings")
        for k, (x, y) in enumerate(zip(have, exp)):
            for field, fx, fy in zip(fc.FIELDS, x, y):
                assert fx == fy, (what, "input", i, "encoding", k, field, case["inputs"][i])
    seqs = fc.decode_sequences(case, [enc[0][0] for enc in rec["enc"]])
    for skip, exp in zip((False, True), rec["dec"]):
        if exp is None:
            continue
        try:
            dec = tok.decode_batch(seqs, skip_special_tokens=skip)
        except ta.UnsupportedError:      # (the decoder, or a normalized added token behind a normalizer, is off the path: refused at the call)
            break
        assert dec == exp, (what, "decode_batch, skip_special_tokens", skip)
    return "compared"


@pytest.mark.parametrize("name", fc.FAMILIES)
def test_family_against_the_wheels_vectors(name):
    outcomes = [hold_case(fc.make_case(name, seed), rec, (name, seed)) for seed, rec in zip(fc.SEEDS, vectors()["families"][name])]
    assert len(outcomes) - outcomes.count("refused") >= 8, outcomes


@pytest.mark.parametrize("finding", sorted(fc.found_cases()))
def test_found(finding):
    for k, (case, rec) in enumerate(zip(fc.found_cases()[finding], vectors()["found"][finding])):
        assert hold_case(case, rec, (finding, k)) == "compared"
