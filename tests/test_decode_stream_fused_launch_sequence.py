"""What the host code enqueues for ONE step of a fused decode stream (tkamd_decode_stream_new with TKAMD_STREAM_FUSED), read from the launch
log of the SIMT emulation like tests/test_launch_sequence.py: no synchronisation and no copy to the host, at most 6 kernel launches and one
memset, and the SAME sequence for ByteLevel, the ByteFallback chain, CTC and WordPiece, whether or not a window holds a cut character --
next to the step of an object that is not fused over the same inputs, whose sequence stays what it was.  Both are compared with the
recorded sequences of tests/golden/launch_sequences_decode_stream_fused.json, this test's own fixture, written by
`python tests/test_decode_stream_fused_launch_sequence.py --record`.  (When it was first recorded, the unfused sequences were also logged
from a build of the commit before the fused step, over the same ids: all eight were equal to the recorded ones.)"""
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

from tests import decode_cases as dc
from tests import test_launch_sequence as base
from tests.helpers import GOLD

simt_library = base.simt_library        # (module-scoped, autouse: ctypes opens the host build)

FIXTURE = os.path.join(GOLD, "launch_sequences_decode_stream_fused.json")
N_STREAMS = 5
# index into tests/decode_cases.py DECODERS
DECODERS = {"bytelevel": 29, "byte_fallback_chain": 7, "ctc": 13, "wordpiece": 0}
NAMES = [f"{d}_{w}" for d in DECODERS for w in ("plain", "cut")]


def _ids(case, cut):
    """three steps of N_STREAMS ids: words, and -- cut -- the first bytes of a three-byte character in stream 1's window at the third"""
    w = case.words
    rows = [[w[(7 * j + i) % len(w)] for i in range(N_STREAMS)] for j in range(3)]
    if cut:
        if case.byte_id and len(case.byte_id) == 256:          # <0xE2> <0x82>: a run that is not UTF-8 yet
            rows[1][1], rows[2][1] = case.byte_id[0xE2], case.byte_id[0x82]
        elif case.decoder and case.decoder.get("type") == "ByteLevel":
            lone = [i for i, t in case.id2tok.items() if t == "â"]     # the byte-level char of E2 on its own: an invalid subpart
            assert lone, "the ByteLevel fixture has no token for the byte E2"
            rows[1][1] = rows[2][1] = lone[0]
    return rows


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


_loaded = {}


def step_sequences(name):
    """(log of the third step of a fused object, log of the third step of one that is not) over the same ids"""
    import tokenizers_amd as ta
    dec, cut = name.rsplit("_", 1)
    if dec not in _loaded:
        case = dc.Case(DECODERS[dec])
        _loaded[dec] = (case, ta.Tokenizer.from_str(case.json, device=0))
    case, tok = _loaded[dec]
    rows = [np.asarray(r, dtype=np.uint32) for r in _ids(case, cut == "cut")]
    out = []
    for fused in (True, False):
        ds = tok.decode_stream(N_STREAMS, skip_special_tokens=False, window=8, fused=fused)
        assert ds.fused is fused
        for r in rows[:2]:
            ds.step_device(r.ctypes.data, 0, "uint32")
        got = []
        out.append(_log(lambda: got.append(ds.step_device(rows[2].ctypes.data, 0, "uint32")[0])))
        if cut == "cut" and dec in ("bytelevel", "byte_fallback_chain"):
            _, _, status = ds.read(got[0])
            assert status[1] == 0 and 1 in list(status), status  # the cut character holds its stream back, others emit
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)["cases"]


@pytest.fixture(scope="module")
def logs():
    return {name: step_sequences(name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_a_fused_step_only_enqueues(name, logs, recorded):
    fused, _ = logs[name]
    assert not [l for l in fused if l.startswith("sync")], fused
    assert not [l for l in fused if l.startswith("memcpy")], fused            # (device ids in: nothing is copied either way)
    launches = [l for l in fused if l.startswith("launch ")]
    assert 1 <= len(launches) <= 6 and len([l for l in fused if l.startswith("memset")]) <= 1, fused
    assert len(launches) + len([l for l in fused if l.startswith("memset")]) == len(fused), fused
    assert any("k_ds_step_fused" in l for l in launches) and not any("k_decode_" in l or "k_lossy_" in l for l in launches), fused
    assert fused == recorded[name]["fused"]


def test_the_fused_sequence_is_one_for_every_decoder_and_window(logs):
    first = logs[NAMES[0]][0]
    for name in NAMES:
        assert logs[name][0] == first, name


@pytest.mark.parametrize("name", NAMES)
def test_an_unfused_step_logs_what_it_logged(name, logs, recorded):
    """the step of an object made without the flag: the recorded sequence of the range decode's launches and waits, untouched"""
    _, plain = logs[name]
    assert plain == recorded[name]["unfused"]
    assert len([l for l in plain if l.startswith("sync")]) >= 3 and not any("k_ds_step_fused" in l for l in plain)


if __name__ == "__main__":
    from tests.harness import simt_build
    simt_build.build()
    _lib.LIB_PATH, _lib._lib = simt_build.SO, None
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_decode_stream_fused_launch_sequence.py --record"
    cases = {}
    for name in NAMES:
        f, u = step_sequences(name)
        cases[name] = {"fused": f, "unfused": u}
    out = {"_about": "RECORDED RESULT: the launch log of tests/test_decode_stream_fused_launch_sequence.py, written by its --record; record it again "
                     "only for a change that moves a launch of a decode stream step on purpose",
           "cases": cases}
    with open(FIXTURE, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=0, ensure_ascii=True)
        fh.write("\n")
    print({k: (len(v["fused"]), len(v["unfused"])) for k, v in cases.items()})
