"""The seeded cross-layout differential (tests/fuzz_cases.py), CPU half: the generator still makes the cases the vectors were recorded for
(by SHA-256: a drift is a failure, not a silent change of tests/test_fuzz_layouts_gpu.py), the wheel -- where it imports -- still answers
what tools/make_golden_fuzz.py recorded, and at least 8 of every family's 12 cases load and are compared."""
import pytest

from tests import fuzz_cases as fc
from tests.fuzz_cases import vectors


def wheel_answers(ref, case):
    """what tools/make_golden_fuzz.py records of the wheel: (raised, enc, dec)"""
    rt = ref.Tokenizer.from_str(case["json"])
    rt.encode_special_tokens = case["encode_special_tokens"]
    try:
        exp = rt.encode_batch(fc.call_inputs(case), add_special_tokens=case["add_special_tokens"], is_pretokenized=case["is_pretokenized"])
    except BaseException:
        return True, None, None
    dec = []
    for skip in (False, True):
        try:
            dec.append(rt.decode_batch(fc.decode_sequences(case, [e.ids for e in exp]), skip_special_tokens=skip))
        except BaseException:
            dec.append(None)
    return False, [fc.deep(e) for e in exp], dec


def test_the_vectors_cover_every_family_and_seed():
    v = vectors()
    assert sorted(v["families"]) == fc.FAMILIES and len(fc.FAMILIES) == 44 and not set(fc.FAMILIES) & set(fc.HEAVY)
    assert v["seeds"] == list(fc.SEEDS) == list(range(12))
    assert all(len(recs) == len(fc.SEEDS) for recs in v["families"].values())
    found = fc.found_cases()
    assert sorted(v["found"]) == sorted(found) and all(len(v["found"][k]) == len(found[k]) for k in found)


@pytest.mark.parametrize("name", fc.FAMILIES)
def test_generator_makes_the_recorded_cases(name):
    for seed, rec in zip(fc.SEEDS, vectors()["families"][name]):
        case = fc.make_case(name, seed)
        assert fc.digest(case) == rec["digest"], (name, seed)
        assert 1 <= len(case["inputs"]) <= fc.MAX_DOCS and fc.digest(fc.make_case(name, seed)) == rec["digest"]


@pytest.mark.parametrize("name", fc.FAMILIES)
def test_at_least_8_of_12_cases_load_and_are_compared(name):
    recs = vectors()["families"][name]
    assert sum(1 for r in recs if r["refused"] is None) >= 8, [r["refused"] for r in recs]
    assert all(r["refused"] is not None or r["raised"] or r["enc"] is not None for r in recs)


@pytest.mark.parametrize("name", fc.FAMILIES)
def test_wheel_answers_what_was_recorded(ref_tokenizers, name):
    for seed, rec in zip(fc.SEEDS, vectors()["families"][name]):
        raised, enc, dec = wheel_answers(ref_tokenizers, fc.make_case(name, seed))
        assert raised == rec["raised"], (name, seed)
        assert enc == rec["enc"], (name, seed)
        assert dec == rec["dec"], (name, seed)


@pytest.mark.parametrize("finding", sorted(fc.found_cases()))
def test_found_cases_are_the_recorded_ones(finding):
    for k, (case, rec) in enumerate(zip(fc.found_cases()[finding], vectors()["found"][finding])):
        assert fc.digest(case) == rec["digest"], (finding, k)
        assert rec["refused"] is None and not rec["raised"], (finding, k)


@pytest.mark.parametrize("finding", sorted(fc.found_cases()))
def test_wheel_answers_the_found_cases_as_recorded(ref_tokenizers, finding):
    for k, (case, rec) in enumerate(zip(fc.found_cases()[finding], vectors()["found"][finding])):
        assert wheel_answers(ref_tokenizers, case) == (rec["raised"], rec["enc"], rec["dec"]), (finding, k)
