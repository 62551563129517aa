"""What a load produces, pinned (CPU, no GPU): tests/harness/host_model_digest.cpp is built with g++ next to
tokenizers_amd/csrc/host_model.cpp and run over the corpus of tests/host_model_cases.py; every file's outcome -- loaded, with the
digests of what the load configured and of what its tables hold, or refused, with the whole message -- is held to
tests/golden/host_model_outcomes.json.gz (tools/make_golden_host_model.py) exactly.  The two-fault files pin WHICH refusal a file
with two faults gets: the order of the loader's questions.  A sanitizer build of the same program answers the small files alike."""
import gzip
import json
import os

import pytest

from tests import fuzz_cases as fc
from tests import host_model_cases as hc
from tests.helpers import GOLD


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(GOLD, "host_model_outcomes.json.gz"), "rt", encoding="utf-8") as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def harness_exe(tmp_path_factory):
    return hc.build_harness(str(tmp_path_factory.mktemp("host_model_digest") / "host_model_digest"))


def test_corpus_and_golden_file_have_the_same_keys(golden):
    keys = [k for make in hc.GROUPS.values() for k, _ in make()]
    assert len(keys) == len(set(keys))
    assert sorted(keys) == sorted(golden)
    assert len(hc.FIXTURES) == 51 and sum(1 for k in keys if k.startswith("two_fault/")) >= 16
    assert sum(1 for k in keys if k.startswith("fuzz/")) == 44 * 12


@pytest.mark.parametrize("group", list(hc.GROUPS))
def test_load_outcomes_are_the_recorded_ones(group, harness_exe, golden, tmp_path):
    """one fixture with its twelve seeded edits (a HEAVY fixture alone); the found cases; the two-fault files"""
    items = list(hc.GROUPS[group]())
    got = hc.run_harness(harness_exe, items, str(tmp_path), jobs=1)
    for key, _ in items:
        assert got[key] == golden[key], key


def test_every_two_fault_file_is_refused(golden):
    """(of the recorded answers: a two-fault file that loaded would pin nothing)"""
    for key, rec in golden.items():
        if key.startswith("two_fault/"):
            assert rec["status"] in ("UNSUPPORTED", "INVALID"), key


def test_sanitizer_build_answers_the_small_files_alike(harness_exe, golden, tmp_path):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer, a stand-alone build: the fixtures but the seven HEAVY ones,
    and the two-fault list; it prints the lines the plain build prints"""
    exe = hc.build_harness(str(tmp_path / "host_model_digest_san"), flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    items = [(f"fixture/{name}", hc.load_tokenizer_json(name)) for name in hc.FIXTURES if name not in fc.HEAVY] + list(hc.GROUPS["two_fault"]())
    (tmp_path / "plain").mkdir()
    (tmp_path / "san").mkdir()
    plain = hc.run_harness(harness_exe, items, str(tmp_path / "plain"), jobs=1)
    assert hc.run_harness(exe, items, str(tmp_path / "san"), jobs=2) == plain
    assert plain == {k: golden[k] for k, _ in items}
