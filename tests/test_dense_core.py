"""CPU test of the dense stage's per-element decision: csrc/dense_core.hpp, the header k_dense_rows calls for every element, compiled
for the host and walked by tests/harness/dense_harness.cpp over every (n_tokens, pad, side, n_prefix, n_suffix, width <= 9), with and
without sequence ids.  The harness checks memory safety itself (it is built with -fsanitize=address,undefined and reads the row's
arrays, heap blocks of exactly the row, through the indices it gets); this test holds every shape the pipeline can make -- and the
too-short rows it cannot -- to a restatement of the layout as a list, the way Encoding._mask builds it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "harness", "dense_harness.cpp")
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")
MAX_WIDTH = 9


def restated(n, pad, left, n_prefix, n_suffix, width):
    """the row as a list -- padding, special tokens, the sequence, special tokens, padding -- cut or filled up to `width` columns"""
    body = ["S"] * n_prefix + ["T"] * (n - pad - n_prefix - n_suffix) + ["S"] * n_suffix
    row = ["P"] * pad + body if left else body + ["P"] * pad
    assert len(row) == n
    cols = ["%s%d" % (k, c) for c, k in enumerate(row[:width])]
    return ",".join(cols + ["P-"] * (width - len(cols)))


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler here")
    exe = str(tmp_path_factory.mktemp("dense") / "dense_harness")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(MAX_WIDTH)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok: "), lines[-1]
    out = {}
    for line in lines[:-1]:
        head, cols = line.split("|")
        out[tuple(int(x) for x in head.split())] = cols
    assert len(out) == len(lines) - 1 == int(lines[-1].split()[1])
    return out


def test_every_row_shape_is_the_restated_layout(walked):
    checked = 0
    for (n, pad, left, n_prefix, n_suffix, width, with_seq), cols in walked.items():
        if pad > n or n_prefix + n_suffix > n - pad:
            continue                                         # (no such row: safety only, below)
        if n > width and (left or pad or n_suffix):
            continue                                         # (a row that is too long is cut where it is read; what its tail held is not laid out)
        assert cols == restated(n, pad, left, n_prefix, n_suffix, width), (n, pad, left, n_prefix, n_suffix, width, with_seq)
        checked += 1
    assert checked > 4000
    # the shapes the pipeline makes: exactly `width` tokens
    assert walked[(5, 2, 1, 1, 1, 5, 0)] == "P0,P1,S2,T3,S4" and walked[(5, 2, 0, 1, 1, 5, 1)] == "S0,T1,S2,P3,P4"
    assert walked[(4, 4, 0, 0, 0, 4, 0)] == "P0,P1,P2,P3" and walked[(3, 0, 0, 0, 0, 3, 0)] == "T0,T1,T2"


def test_no_shape_reads_outside_its_row(walked):
    """every answer names its own column of the row or nothing, never more columns than the row has tokens or the output has columns"""
    for (n, pad, left, n_prefix, n_suffix, width, with_seq), cols in walked.items():
        parts = cols.split(",")
        assert len(parts) == width
        for c, p in enumerate(parts):
            assert p[0] in "TSP"
            if c < min(n, width):
                assert p[1:] == str(c)
            else:
                assert p == "P-"
