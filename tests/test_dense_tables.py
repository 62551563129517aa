"""The densely packed short-word and merge tables (tests/dense_tables_cases.py) without a GPU: the whole device path compiled for the
host under the SIMT shim, as in tests/test_simt_pipeline.py.  The same checks run on the MI355X in tests/test_dense_tables_gpu.py, with
the vocabulary at the size where 16,384 buckets are needed."""
import pytest

from oracle import synth
from tokenizers_amd import _lib

from tests import dense_tables_cases as D
from tests.harness import simt_build


@pytest.fixture(scope="module", autouse=True)
def simt_library():
    """ctypes opens the host build for the tests of this module (handles made before and after keep their own library)"""
    simt_build.build()
    saved = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    try:
        yield
    finally:
        _lib.LIB_PATH, _lib._lib = saved


def test_wordlevel_vocabulary_in_a_table_95_percent_full():
    """3,900 words (+ the unk token) in 4,096 slots: every word is answered with its id, every stranger with the unk id -- among them
    1,000 that differ from a word only in bytes 12..15 -- and the placement needed a displacement beyond eight bits."""
    js, shape = D.check_wordlevel(3900, 4096)
    D.check_determinism(js, shape)


def test_c2_tokenizer_on_the_dense_tables():
    """(the load-time proof of the 50 k vocabulary runs the merge kernel in the emulation: most of this test's time is the load)"""
    D.check_c2(synth.load_or_train_gpt2())
