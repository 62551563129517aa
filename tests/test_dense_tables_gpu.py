"""-m gpu: the densely packed short-word and merge tables (tests/dense_tables_cases.py) on the device."""
import pytest

from oracle import synth

from tests import dense_tables_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpt2_json():
    return synth.load_or_train_gpt2()


def test_wordlevel_vocabulary_in_a_table_95_percent_full():
    """62,000 words (+ the unk token) in 65,536 slots -- 8,192 buckets do not place them, 16,384 do: every word is answered with its id,
    every stranger with the unk id -- among them 1,000 that differ from a word only in bytes 12..15 -- and the placement needed a
    displacement beyond eight bits."""
    js, shape = D.check_wordlevel(62000, 65536)
    D.check_determinism(js, shape)


def test_c2_tokenizer_on_the_dense_tables(gpt2_json):
    shape = D.check_c2(gpt2_json)
    D.check_determinism(gpt2_json, shape)
