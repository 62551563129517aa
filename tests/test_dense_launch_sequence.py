"""What the host code enqueues for ONE call of the dense entry (tkamd_encode_batch_device_dense), read from the launch log of the SIMT
emulation like tests/test_launch_sequence.py: no synchronisation and no copy in either direction, k_dense_rows as the last launch, and in
front of it exactly what tkamd_encode_batch_device enqueues for the same batch with the same flags plus TKAMD_NO_SPECULATION -- the stage
is one launch behind an epilogue that does not move.  A single-sequence configuration (BertProcessing, padded on the left, char offsets and
word ids) and a pair configuration.  Both logs are compared with the recorded sequences of tests/golden/launch_sequences_dense.json, this
test's own fixture, written by `python tests/test_dense_launch_sequence.py --record`."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tokenizers_amd import _lib

from tests import dense_cases as dn
from tests import test_launch_sequence as base
from tests.helpers import GOLD

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

FIXTURE = os.path.join(GOLD, "launch_sequences_dense.json")
NAMES = ["left_padding", "pairs_bert_longest_left"]


def _log(fn):
    lib = _lib.load()
    lib.simt_launch_log_read.restype = C.c_size_t
    lib.simt_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
    lib.simt_launch_log_clear()
    fn()
    n = lib.simt_launch_log_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.simt_launch_log_read(buf, n)
    return buf.raw[:n].decode().splitlines()


def call_sequences(name):
    """(log of a dense call, log of the plain device call with the same flags + TKAMD_NO_SPECULATION) on one handle, each behind a
    first call of its kind; the arrays are numpy memory"""
    import tokenizers_amd as ta
    case = dn.BY_NAME[name]
    tok = ta.Tokenizer.from_str(dn.tokenizer_json(case), device=0)
    docs = [s for it in case["inputs"] for s in it] if case["pairs"] else list(case["inputs"])
    buf, off = ta.pack_documents(docs)
    buf, off = np.array(buf), np.array(off)
    n_rows, width = len(case["inputs"]), case["width"]
    outs = {k: np.zeros((n_rows, width, 2) if k == "offset_mapping" else (n_rows, width), dtype=np.int64) for k in dn.FIELDS}
    flags = tok._dense_flags("char", True, case["add_special_tokens"], case["pairs"])
    res = _lib.DeviceResult()

    def dense():
        tok.encode_batch_device_dense(buf.ctypes.data, off.ctypes.data, len(docs), int(off[-1]), {k: v.ctypes.data for k, v in outs.items()}, width,
                                      pairs=case["pairs"], add_special_tokens=case["add_special_tokens"], offsets="char", word_ids=True)

    def plain():
        _lib.check(tok._lib.tkamd_encode_batch_device(tok._h, buf.ctypes.data, off.ctypes.data, len(docs), int(off[-1]),
                                                      flags | _lib.NO_SPECULATION, 0, C.byref(res)))
    dense()
    d = _log(dense)
    assert outs["attention_mask"].sum() > 0
    plain()
    p = _log(plain)
    return d, p


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


@pytest.fixture(scope="module")
def logs():
    return {name: call_sequences(name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_a_dense_call_only_enqueues(name, logs, recorded):
    dense, _ = logs[name]
    assert not [l for l in dense if l.startswith("sync")], dense
    assert not [l for l in dense if l.startswith("memcpy")], dense
    assert dense[-1].startswith("launch (k_dense_rows<int64_t>) "), dense[-3:]
    assert len([l for l in dense if "k_dense_rows" in l]) == 1
    assert dense == recorded[name]["dense"]


@pytest.mark.parametrize("name", NAMES)
def test_the_stage_is_one_launch_behind_the_plain_call(name, logs, recorded):
    dense, plain = logs[name]
    assert dense[:-1] == plain
    assert plain == recorded[name]["plain"] and not any("k_dense_rows" in l for l in plain)


if __name__ == "__main__":
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_dense_launch_sequence.py --record"
    cases = {}
    for name in NAMES:
        d, p = call_sequences(name)
        cases[name] = {"dense": d, "plain": p}
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_dense_launch_sequence.py, written by its --record; record it again only "
                     "for a change that moves a launch of the dense entry on purpose",
           "cases": cases}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: (len(v["dense"]), len(v["plain"])) for k, v in cases.items()})
