"""CPU tests of the lossy UTF-8 repair behind the device entry of decode_batch: tkamd_probe_utf8_lossy runs the per-byte decision of
csrc/utf8_lossy_core.hpp -- the very function k_lossy_count / k_lossy_len call -- over one sequence on the host.  It is held to
Python's bytes.decode("utf-8", "replace") exhaustively where that is feasible, and Python's "replace" is held to the reference
wheel's ByteLevel decoder (String::from_utf8_lossy, pre_tokenizers/byte_level.rs:170) on the random set."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tokenizers_amd as ta
from tokenizers_amd import _lib
from tests.helpers import load_tokenizer_json

# every class of byte the decision tells apart, at the edges of its range: ASCII, the continuation ranges the restricted leads split
# (80..8F, 90..9F, A0..BF), the bytes that never occur (C1, F5, FF), two-, three- and four-byte leads with and without a restriction
ALPHABET = bytes([0x41, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xED, 0xEE, 0xF0, 0xF1, 0xF4, 0xF5, 0xFF])


def _probe(lib, raw: bytes) -> bytes:
    cap = 3 * len(raw) + 1
    out, n = (C.c_uint8 * cap)(), C.c_int64(-1)
    assert lib.tkamd_probe_utf8_lossy(raw, len(raw), out, cap, C.byref(n)) == _lib.OK, raw
    return bytes(out[:n.value])


def _expect(raw: bytes) -> bytes:
    return raw.decode("utf-8", "replace").encode("utf-8")


def _check_all(strings):
    lib = _lib.load()
    got = ((s, _probe(lib, s), _expect(s)) for s in strings)
    bad = [(s.hex(), g.hex(), e.hex()) for s, g, e in got if g != e]
    assert not bad, f"{len(bad)} strings differ, first (input, got, expected) {bad[0]}"


def _random_strings():
    rng = np.random.default_rng(170)
    return [bytes(ALPHABET[int(j)] for j in rng.integers(0, len(ALPHABET), size=int(n))) for n in rng.integers(1, 13, size=20_000)]


def test_every_one_byte_string():
    _check_all([bytes([a]) for a in range(256)])


def test_every_two_byte_string():
    _check_all([bytes([a, b]) for a in range(256) for b in range(256)])


@pytest.mark.parametrize("n", [3, 4])
def test_every_string_over_the_alphabet(n):
    _check_all([bytes(t) for t in itertools.product(ALPHABET, repeat=n)])


def test_random_strings_over_the_alphabet():
    _check_all(_random_strings())


def test_python_replace_is_the_reference_lossy(ref_tokenizers):
    """The assumption the tests above (and Tokenizer.decode_batch) rest on, held to the reference itself: the wheel's ByteLevel decoder
    over one token per byte -- from_utf8_lossy of exactly these bytes -- against the probe and against Python's "replace"."""
    from oracle.decode_oracle import bytes_char
    b2c = bytes_char()
    dec = ref_tokenizers.decoders.ByteLevel()
    lib = _lib.load()
    for s in _random_strings():
        want = dec.decode([b2c[b] for b in s])
        assert want == s.decode("utf-8", "replace"), s.hex()
        assert _probe(lib, s).decode("utf-8") == want, s.hex()


def test_probe_edges():
    lib = _lib.load()
    n = C.c_int64(-1)
    assert lib.tkamd_probe_utf8_lossy(None, 0, None, 0, C.byref(n)) == _lib.OK and n.value == 0
    out = (C.c_uint8 * 2)()
    assert lib.tkamd_probe_utf8_lossy(b"\xff", 1, out, 2, C.byref(n)) == _lib.ERR_INVALID and n.value == 3      # too small: the size is still told
    assert lib.tkamd_probe_utf8_lossy(b"a", 1, out, 2, None) == _lib.ERR_INVALID
    # a sequence is repaired on its own: E2 82 | AC are two invalid subparts, E2 82 AC is a character
    assert _probe(lib, b"\xe2\x82") == b"\xef\xbf\xbd" and _probe(lib, b"\xac") == b"\xef\xbf\xbd" and _probe(lib, b"\xe2\x82\xac") == b"\xe2\x82\xac"


def test_host_only_handle_has_no_device_decode():
    t = ta.Tokenizer.from_str(load_tokenizer_json("gpt2_synth_50257"), device=-1)
    ids = np.array([1, 2, 3], dtype=np.uint32)
    begin, end = np.array([0], dtype=np.int64), np.array([3], dtype=np.int64)
    res = _lib.DeviceText()
    rc = t._lib.tkamd_decode_batch_device(t._h, ids.ctypes.data, 3, begin.ctypes.data, end.ctypes.data, 1, 0, None, C.byref(res))
    assert rc == _lib.ERR_DEVICE
    with pytest.raises(ta.DeviceError, match="no CPU fallback"):
        t.decode_batch_device(ids.ctypes.data, 3, begin.ctypes.data, end.ctypes.data, 1)
