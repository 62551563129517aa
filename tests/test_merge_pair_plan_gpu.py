"""-m gpu: every boundary of the plan of k_bpe_merge_lds_pair (csrc/merge_pair_plan_core.hpp) on the device, within a few thousand words.

The test hook TKAMD_MERGE_PAIR_GRID (read when the handle is made, like TKAMD_CP_GRID) launches the pair kernel on 4 workgroups where
the product's grid is two a CU.  With that grid a queue of a few hundred words decides the plan: the long role's units of 64, 128, 192
and 256 words -- whole wavefronts, at most one to a SIMD -- and of 320 where the free slots do not suffice; exactly one round, and one
unit more than a round (full units, the overflow dealt in reverse); either queue alone; and the lengths 16 / 17 / 32 at the queues'
borders.  That the hook took effect is read from the device side: Tokenizer.queue_sizes()["merge_pair_grid"] is the grid the batch's pair
launch was given (tkamd_profile_counters out[22]) and must be 4.  What each case expects of the plan is computed here from the queue sizes
the run reports, by the header's rules written out again, so that a case whose words miss the boundary it is named for fails instead
of testing something else.

Every case is compared with the CPU oracle document by document (ids; byte offsets + word ids) and run again with TKAMD_MERGE_PAIR=0,
which must give identical arrays (tests/test_merge_pair_gpu.py::_check, used as it is)."""
import pytest

from oracle import oracle as orc
from oracle import synth
from tests.test_merge_pair_gpu import _check, _hooks, _lines, _random_words

pytestmark = pytest.mark.gpu

GRID = 4


@pytest.fixture(scope="module")
def gpt2_small_grid():
    import tokenizers_amd as ta
    js = synth.load_or_train_gpt2()
    with _hooks(TKAMD_CLAIMS_PAUSE="0", TKAMD_MERGE_PAIR_GRID=str(GRID)):
        tok = ta.Tokenizer.from_str(js, device=0)
    return tok, orc.Oracle(js)


def _plan(n16, n32, grid=GRID):
    """(rounds, take_l, take_s) by the rules of merge_pair_plan_core.hpp"""
    up64 = lambda x: (x + 63) // 64 * 64
    need_l, need_s = -(-n32 // 320), -(-n16 // 640)
    rounds = -(-(need_l + need_s) // grid)
    take_l, take_s = 320, 640
    if rounds == 1:
        if n32:
            thin = up64(-(-n32 // (grid - need_s)))
            take_l = thin if thin <= 256 else 320
        if n16:
            take_s = min(640, up64(-(-n16 // (grid - -(-n32 // take_l)))))
    return rounds, take_l, take_s


def _docs(n_short, n_long, seed):
    """n_short distinct words of 8..15 letters and n_long of 17..31, a space in front of each but a line's first (their pre-tokens are a
    byte longer: <= 16 and 18..32 bytes)"""
    short = _random_words(n_short, 8, 15, seed=seed) if n_short else []
    long_ = _random_words(n_long, 17, 31, seed=seed + 1) if n_long else []
    return _lines(short) + _lines(long_, per_line=6)


# (short words, long words) -> the plan the case is there for: (rounds, take_l); the short queue's units follow from the rest
CASES = [
    ("long take 64", 700, 100, (1, 64)),           # 2 short units needed, 2 slots free: 100 words over 2 slots
    ("long take 128", 700, 250, (1, 128)),
    ("long take 192", 700, 380, (1, 192)),
    ("long take 256", 700, 500, (1, 256)),
    ("long take 320", 700, 600, (1, 320)),         # 300 a slot: more than four wavefronts -- the fallback
    ("exactly one round", 1280, 640, (1, 320)),    # 2 + 2 full units
    ("one unit more than a round", 1400, 640, (2, 320)),
    ("long only, thin", 0, 900, (1, 256)),
    ("long only, full", 0, 1200, (1, 320)),
    ("long only, two rounds", 0, 1500, (2, 320)),
    ("short only", 1500, 0, (1, 320)),
    ("short only, two rounds", 2700, 0, (2, 320)),
]


@pytest.mark.parametrize("name,n_short,n_long,want", CASES, ids=[c[0].replace(" ", "-").replace(",", "") for c in CASES])
def test_plan_boundary(gpt2_small_grid, name, n_short, n_long, want):
    tok, o = gpt2_small_grid
    q = _check(tok, o, _docs(n_short, n_long, seed=700 + 2 * [c[0] for c in CASES].index(name)))
    # (random letters: no word is in the vocabulary, every one is queued; n_long and n_short ARE the fills)
    assert (q["merge16"], q["merge32"]) == (n_short, n_long), q
    assert q["merge_pair_grid"] == GRID, q                                  # the launch itself ran on the hook's grid
    rounds, take_l, _ = _plan(q["merge16"], q["merge32"])
    assert (rounds, take_l) == want, (name, q, _plan(q["merge16"], q["merge32"]))


def test_lengths_at_the_borders_of_the_queues(gpt2_small_grid):
    """pre-tokens of exactly 15, 16, 17, 18, 31, 32 and 33 bytes, with and without the space in front: the last word of the short queue,
    the first and the last of the long one, and the first that neither takes"""
    tok, o = gpt2_small_grid
    docs = []
    for L in (15, 16, 17, 18, 31, 32, 33):
        ws = _random_words(60, L, L, seed=730 + L)
        docs += ws[:30]
        docs += _lines(["x"] + ws[30:], per_line=8)
    q = _check(tok, o, docs)
    assert q["merge16"] > 0 and q["merge32"] > 0 and q["merge64"] > 0, q
    assert q["merge_pair_grid"] == GRID, q
    assert _plan(q["merge16"], q["merge32"])[0] == 1, q


def test_without_the_hook_the_grid_is_what_is_resident():
    """no hook: the pair launch takes the resident capacity, merge_pair_wg_per_cu workgroups for each of the device's CUs (the launch log
    of tests/test_launch_sequence.py pins the launch byte for byte)"""
    import tokenizers_amd as ta
    js = synth.load_or_train_gpt2()
    with _hooks(TKAMD_CLAIMS_PAUSE="0"):
        tok = ta.Tokenizer.from_str(js, device=0)
    o = orc.Oracle(js)
    q = _check(tok, o, _docs(700, 380, seed=760))
    assert (q["merge16"], q["merge32"]) == (700, 380), q
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else None
    assert q["merge_pair_grid"] >= 1 and q["merge_pair_grid"] % q["merge_pair_wg_per_cu"] == 0, q
    if n_cu:                                                                 # (the emulation has no device to ask)
        assert q["merge_pair_grid"] == n_cu * q["merge_pair_wg_per_cu"], (q, n_cu)
