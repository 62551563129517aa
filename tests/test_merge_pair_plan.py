"""CPU test of the plan of k_bpe_merge_lds_pair: csrc/merge_pair_plan_core.hpp, the header the kernel derives its roles, takes and rounds
from, compiled for the host and walked by tests/harness/merge_pair_plan_harness.cpp over the fills from 0 (either queue empty) to just
past two rounds: every pair of fills for the grids 1, 2, 3 and 8 (66 M plans); for the grid of 512, where that would be 2e11, the fills
within 2 of a multiple of 64 at a stride -- the plan changes nowhere else --, the borders of one and two rounds and C2's fills:

  * every item of both queues belongs to exactly one (round, workgroup, lane);
  * units per round <= grid;
  * takes are multiples of 64, take_s <= 640 and take_l <= 320;
  * take_l <= 256 -- no SIMD runs two 32-symbol wavefronts of a unit -- whenever the slots the short role leaves free allow it, the
    smallest multiple of 64 that fits, and 320 only where they do not;
  * more than one round keeps full units.

The harness is a stand-alone program, built with -fsanitize=address,undefined and run as one."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "harness", "merge_pair_plan_harness.cpp")
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")


def test_plan_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler here")
    exe = str(tmp_path / "merge_pair_plan_harness")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ok: "), r.stdout
    print(r.stdout.strip())
