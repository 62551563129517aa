"""-m gpu: k_bpe_merge_lds_pair, the launch that merges the <= 16-byte queue and the 17..32-byte queue side by side (kernels/bpe.hip).

Every case is compared with the CPU oracle document by document, ids only and with byte offsets + word ids, and is then encoded once
more with the test hook TKAMD_MERGE_PAIR=0 -- the single launch of the 32-symbol kernel that served both queues before -- which must
give identical arrays.  The cases are the shapes the kernel's plan (roles, takes, rounds) is derived from: thin queues, a <= 16-byte
queue of more than one round, either queue alone, none, the lengths at the queues' borders, rows that spill to tmp_ids, and a
tokenizer whose lookup retires whole words first (ignore_merges)."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import synth
from tests.helpers import N

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)


def _random_words(n, lo, hi, seed):
    """n DISTINCT words of lo..hi random lower-case letters (hi >= 8: no vocabulary holds one whole; a counter in base 26 at the front makes
    them distinct)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    raw = LETTERS[rng.integers(0, 26, size=(n, hi))]
    k = np.arange(n)
    for d in range(5):                                   # 26^5 > 11 M
        raw[:, d] = LETTERS[k % 26]
        k = k // 26
    return [raw[i, :lens[i]].tobytes().decode() for i in range(n)]


def _lines(words, per_line=10):
    return [" ".join(words[i:i + per_line]) for i in range(0, len(words), per_line)]


class _hooks:
    def __init__(self, **env):
        self.env = dict(env, TKAMD_TEST_HOOKS="1")

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _tokenizer(js):
    """(a handle that never pauses its in-batch claims -- read at load --: a batch of words that all differ would switch them, and with
    them the pair kernel, off for the handle's next batches)"""
    import tokenizers_amd as ta
    with _hooks(TKAMD_CLAIMS_PAUSE="0"):
        return ta.Tokenizer.from_str(js, device=0)


@pytest.fixture(scope="module")
def gpt2():
    js = synth.load_or_train_gpt2()
    return _tokenizer(js), orc.Oracle(js)


def _first_bad_doc(got_off, got, exp_off, exp):
    for d in range(len(exp_off) - 1):
        if got_off[d] != exp_off[d] or got_off[d + 1] != exp_off[d + 1] or not np.array_equal(got[got_off[d]:got_off[d + 1]], exp[exp_off[d]:exp_off[d + 1]]):
            return d
    return -1


def _check(tok, oracle, docs):
    """ids only and ids + byte offsets + word ids against the oracle, per document; then the same two calls with the pair kernel off.
    Returns the queue sizes of the pair-kernel run."""
    exp = oracle.encode_batch(docs)
    exp_off = np.asarray(exp.tok_offsets)
    tok.profile(True)
    fast = tok.encode_batch_fast(docs, add_special_tokens=False)
    tok.profile(False)
    stages = tok.profile_read()
    q = tok.queue_sizes()
    assert "bpe_merge_lds_pair" in stages and "bpe_merge_lds32" not in stages and "bpe_merge_lds" not in stages, sorted(stages)
    full = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    for name, got in (("ids only", fast), ("with offsets", full)):
        got_off = np.asarray(got.tok_offsets)
        bad = _first_bad_doc(got_off, np.asarray(got.ids), exp_off, np.asarray(exp.ids))
        assert bad < 0, f"{name}: ids of document {bad} {docs[bad][:80]!r}"
        assert np.array_equal(got_off, exp_off)
    off_got, off_exp = np.asarray(full.offsets).reshape(len(exp.ids), -1), np.asarray(exp.offsets).reshape(len(exp.ids), -1)
    bad = _first_bad_doc(exp_off, off_got, exp_off, off_exp)
    assert bad < 0, f"byte offsets of document {bad} {docs[bad][:80]!r}"
    bad = _first_bad_doc(exp_off, np.asarray(full.word_ids), exp_off, np.asarray(exp.words))
    assert bad < 0, f"word ids of document {bad} {docs[bad][:80]!r}"
    with _hooks(TKAMD_MERGE_PAIR="0"):
        tok.profile(True)
        fast0 = tok.encode_batch_fast(docs, add_special_tokens=False)
        tok.profile(False)
        stages0 = tok.profile_read()
        full0 = tok.encode_batch_csr(docs, offsets="byte", word_ids=True)
    assert "bpe_merge_lds32" in stages0 and "bpe_merge_lds_pair" not in stages0, sorted(stages0)
    assert np.array_equal(np.asarray(fast0.ids), np.asarray(fast.ids)) and np.array_equal(np.asarray(fast0.tok_offsets), np.asarray(fast.tok_offsets))
    assert np.array_equal(np.asarray(full0.ids), np.asarray(full.ids)) and np.array_equal(np.asarray(full0.tok_offsets), np.asarray(full.tok_offsets))
    assert np.array_equal(np.asarray(full0.offsets), np.asarray(full.offsets)) and np.array_equal(np.asarray(full0.word_ids), np.asarray(full.word_ids))
    return q


def test_thin_queues_prose(gpt2):
    tok, o = gpt2
    q = _check(tok, o, synth.gen_lines(N(200000), text_seed=301))
    assert q["merge16"] > 0 and q["merge32"] > 0, q


def test_short_queue_of_more_than_one_round(gpt2):
    """More than 400 k distinct words of <= 16 bytes: beyond what 2 x 256 workgroups of 640 lanes hold at once."""
    tok, o = gpt2
    words = _random_words(N(450000), 8, 15, seed=302)
    q = _check(tok, o, _lines(words))
    assert q["merge16"] > N(400000), q


def test_both_roles_over_more_than_one_round(gpt2):
    """About 300 k distinct short and 40 k distinct long words: more units (469 + 125) than the 512 resident workgroups, so the second
    round, dealt in reverse, hands workgroups that ran a unit of one role (a key area of 320 columns) a unit of the other (640)."""
    tok, o = gpt2
    short, long_ = _random_words(N(300000), 8, 15, seed=308), _random_words(N(40000), 17, 31, seed=309)
    docs = _lines(short) + _lines(long_, per_line=6)
    np.random.default_rng(308).shuffle(docs)
    q = _check(tok, o, docs)
    assert q["merge16"] >= len(short) and q["merge32"] >= len(long_), q
    units = -(-q["merge16"] // 640) + -(-q["merge32"] // 320)
    if q["merge16"] >= 300000:                                  # (the full-size run)
        assert units > 2 * 256, (units, q)


def test_two_workgroups_per_cu_are_resident(gpt2):
    """The launch shape the kernel is laid out for: the runtime's occupancy answer for both instantiations (prepare_pair_merge)."""
    tok, _ = gpt2
    tok.encode_batch_fast(["one batch"], add_special_tokens=False)
    import torch
    if torch.cuda.is_available():                               # (the emulation's occupancy query answers 1)
        assert tok.queue_sizes()["merge_pair_wg_per_cu"] == 2


def test_only_long_words(gpt2):
    tok, o = gpt2
    words = _random_words(N(60000), 17, 31, seed=303)
    q = _check(tok, o, _lines(words, per_line=6))
    assert q["merge16"] == 0 and q["merge32"] >= len(words), q


def test_only_short_words(gpt2):
    tok, o = gpt2
    words = _random_words(N(60000), 8, 15, seed=304)
    q = _check(tok, o, _lines(words))
    assert q["merge32"] == 0 and q["merge16"] >= len(words), q


def test_both_queues_empty(gpt2):
    tok, o = gpt2
    docs = ["a", "", " ", "b", "x", "1", "\n", "."] * N(2000, floor=50)     # (a byte is a word of the vocabulary: the lookup retires it)
    q = _check(tok, o, docs)
    assert q["merge16"] == 0 and q["merge32"] == 0, q


def test_lengths_at_the_borders(gpt2):
    """Pre-tokens of exactly 16, 17 and 32 bytes (and their neighbours), with and without the space in front that the GPT-2 split
    glues to a word."""
    tok, o = gpt2
    docs = []
    for L in (15, 16, 17, 18, 31, 32, 33):
        ws = _random_words(N(3000), L, L, seed=310 + L)
        docs += ws[:len(ws) // 2]                                   # a document of one word: L bytes
        docs += _lines(["x"] + ws[len(ws) // 2:], per_line=8)       # behind a space: L + 1 bytes
    q = _check(tok, o, docs)
    assert q["merge16"] > 0 and q["merge32"] > 0 and q["merge64"] > 0, q


def test_rows_of_more_than_four_tokens(gpt2):
    tok, o = gpt2
    rng = np.random.default_rng(305)
    # consonant runs: no merge joins much of them
    cons = np.frombuffer(b"bcdfghjklmnpqrstvwxz", dtype=np.uint8)
    words = [cons[rng.integers(0, len(cons), size=int(L))].tobytes().decode() for L in rng.integers(9, 31, size=N(40000))]
    exp = o.encode_batch(words[:200])
    assert sum(1 for d in range(200) if len(exp.doc_ids(d)) > 4) > 100
    _check(tok, o, _lines(words, per_line=7))


def test_ignore_merges_tokenizer():
    js = synth.load_or_train_llama3()
    tok, o = _tokenizer(js), orc.Oracle(js)
    assert tok.info["ignore_merges"] == 1
    docs = synth.gen_lines(N(60000), text_seed=306, n_types=250000) + _lines(_random_words(N(30000), 6, 31, seed=307)) + synth.stress_lines(seed=23, n=N(2000))
    q = _check(tok, o, docs)
    assert q["merge16"] > 0 and q["merge32"] > 0, q
