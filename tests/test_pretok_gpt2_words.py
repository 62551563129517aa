"""CPU tests of the word-aligned form of tokenizers_amd/csrc/pretok_gpt2_core.hpp -- what a lane of k_pretok_gpt2_seq runs -- through
tests/harness/g2w_harness.cpp: the start mask and the lead mask, computed lane by lane with the halos passed the way the kernel passes
them, are word for word those of gpt2_lane_starts (the window form, which tests/test_pretok_core.py holds against the oracle)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gpt2_word_cases as gc
from tests import word_edge_totals as wt
from tests.helpers import load_tokenizer_json

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "g2w_harness.cpp"), os.path.join(CSRC, "host_model.cpp")]
INCS = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SO = os.path.join(HERE, "harness", "_g2w_harness.so")


@pytest.fixture(scope="module")
def harness():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("pretok_gpt2_core.hpp", "tables.hpp", "host_model.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCS + SRCS + ["-o", tmp], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.g2w_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    lib.g2w_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def js():
    return load_tokenizer_json("gpt2_synth_50257").encode("utf-8")


def _pack(docs):
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return b"".join(raw), off


def _same(lib, js, text, off):
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = int(off[-1])
    assert n == len(text)
    buf = np.frombuffer(text + b"\0", dtype=np.uint8).copy()
    nw = (n >> 6) + 1
    sn, ln, so, lo = (np.zeros(nw, dtype=np.uint64) for _ in range(4))
    assert lib.g2w_run(js, len(js), buf.ctypes.data, n, off.ctypes.data, len(off) - 1, sn.ctypes.data, ln.ctypes.data, so.ctypes.data, lo.ctypes.data) == 0
    for what, new, old in (("start", sn, so), ("lead", ln, lo)):
        bad = np.nonzero(new != old)[0]
        if len(bad):
            w = int(bad[0])
            raise AssertionError(f"{what} mask: {len(bad)} of {nw} words differ; first is word {w} (bytes {64 * w}..): new {int(new[w]):016x} "
                                 f"old {int(old[w]):016x}, text {text[max(0, 64 * w - 8):64 * w + 72]!r}")
    assert so.any() or n == 0


def test_words_equal_windows_on_random_documents(harness, js):
    """300,000 short documents and 6,000 long ones over the adversarial alphabet: every kind of byte falls on every offset of a word, and
    at 6 MB of text some four hundred workgroup edges and fifteen hundred wavefront edges are crossed."""
    for seed in range(3):
        _same(harness, js, *_pack(gc.random_docs(100000, 700 + seed, max_len=40)))
    _same(harness, js, *_pack(gc.random_docs(6000, 710, max_len=400)))


@pytest.mark.parametrize("kind", ["lane", "wave", "group"])
def test_words_equal_windows_on_straddling_cases(harness, js, kind):
    """a multi-byte code point, a contraction, spaces in front of a letter and a document start at every offset from 8 bytes in front of
    an edge to 8 behind it (for a lane edge: byte offsets 56..72 of a word), for the edges between two lanes, two wavefronts (4,096
    bytes) and two workgroups (16,384 bytes)"""
    text, off = gc.straddling_text(gc.edges_of(kind))
    _same(harness, js, text, off)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 17])
def test_words_equal_windows_at_text_lengths(harness, js, n):
    """the text ends on, just before and just behind every kind of edge; documents end wherever they end"""
    docs, total = [], 0
    for d in gc.random_docs(4000, 720 + n % 7, max_len=60):
        b = len(d.encode("utf-8"))
        if total + b > n:
            break
        docs.append(d)
        total += b
    docs.append("x" * (n - total))
    _same(harness, js, *_pack(docs))


@pytest.mark.parametrize("total", wt.TOTALS)
def test_words_equal_windows_at_the_workgroup_edge_in_one_document_and_two(harness, js, total):
    """the text's last word and the edge of a workgroup together, without a document edge near them"""
    for docs in wt.batches(total):
        _same(harness, js, *_pack(docs))


def test_standalone_program_under_sanitizers(js, tmp_path):
    """the same comparison by the harness built as a program of its own with -fsanitize=address,undefined: no load or shift of the new
    functions leaves its buffer or its type's range (the text buffer ends with the 64 bytes of pad the device's has, and at most 15 more)"""
    exe = str(tmp_path / "g2w_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DG2W_STANDALONE"] + INCS + SRCS + ["-o", exe],
                   check=True)
    (tmp_path / "tok.json").write_bytes(js)
    lane_text, lane_off = gc.straddling_text(gc.edges_of("lane"))
    wave_text, wave_off = gc.straddling_text(gc.edges_of("wave"))
    rnd_text, rnd_off = _pack(gc.random_docs(20000, 730, max_len=40))
    for name, text, off in (("lane", lane_text, lane_off), ("wave", wave_text, wave_off), ("random", rnd_text, rnd_off), ("empty", b"", [0, 0])):
        (tmp_path / f"{name}.bin").write_bytes(text)
        (tmp_path / f"{name}.off").write_bytes(np.asarray(off, dtype="<i8").tobytes())
        r = subprocess.run([exe, str(tmp_path / "tok.json"), str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.off")], capture_output=True, text=True)
        assert r.returncode == 0, f"{name}: {r.stdout[-500:]}{r.stderr[-3000:]}"
