"""The decode oracle (oracle/decode_oracle.py) against the reference wheel on exactly the sequences of tests/decode_cases.py: every
decoder case, both skip_special_tokens values, no input left out.  This is what lets tests/test_decode_gpu.py compare the device with
the oracle alone (the wheel need not be importable where the device is)."""
import pytest

from oracle.decode_oracle import DecodeOracle
from tests import decode_cases as dc

LARGE_TOKENS_HERE = 20_000


@pytest.mark.parametrize("k", range(len(dc.DECODERS)), ids=dc.case_id)
def test_decode_oracle_matches_wheel_on_the_decode_cases(k, ref_tokenizers):
    case = dc.Case(k)
    ref = ref_tokenizers.Tokenizer.from_str(case.json)
    o = DecodeOracle(case.json)
    rng = dc.rng_for(k)
    batches = dc.sequences(case, rng)
    if case.large:
        batches.append(dc.large_batch(case, rng, LARGE_TOKENS_HERE))
    assert sum(b.n_tokens for b in batches) > 16_000 and any(b.featured for b in batches)
    for b in batches:
        for skip in (True, False):
            exp = ref.decode_batch(b.seqs, skip_special_tokens=skip)
            got = o.decode_batch(b.seqs, skip)
            bad = [(i, b.seqs[i][:40], got[i][:80], exp[i][:80]) for i in range(len(exp)) if got[i] != exp[i]]
            assert len(got) == len(exp) and not bad, f"{dc.case_id(k)} {b.name} skip={skip}: {len(bad)} sequences differ, first {bad[0]!r}"


def test_the_cases_are_seeded():
    a, b = dc.Case(7), dc.Case(7)
    assert [x.seqs for x in dc.sequences(a, dc.rng_for(7))] == [x.seqs for x in dc.sequences(b, dc.rng_for(7))]
