"""-m gpu: ONE host-entry call sharded over a device list inside the library (tkamd_tokenizer_from_json_devices,
include/tokenizers_amd.h "one call, every GPU"): the reference's encode_batch is one call that uses every parallel resource
(tokenizer/mod.rs:1345-1348, utils/parallelism.rs:85-106).

On a one-GPU box the list names device 0 several times -- SURVEY section 7's multi-"device" emulation: the same host threads,
streams, shard cuts, displacements and collect code run, the replicas just share a GPU.  Every result must equal the unsharded
call's bit for bit; the oracle pins the unsharded call elsewhere.  RCCL wants distinct devices, so on one GPU its gather runs with
a one-device list (rank 0 sends to and receives from itself through ncclSend / ncclRecv)."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import synth
from tests.helpers import N, load_tokenizer_json

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _small_shards(monkeypatch):
    monkeypatch.setenv("TKAMD_SHARD_MIN_KB", "8")        # (read when a handle is made) the test batches are a few hundred kB


def _devs(n: int) -> list:
    """the device list of an n-shard handle: device 0 named n times (one-GPU boxes; what the driver's gate runs), or -- with
    TKAMD_TEST_DISTINCT_DEVICES=1 on a node that has them, tools/first_contact_multi_gpu.sh -- n distinct GPUs"""
    if os.environ.get("TKAMD_TEST_DISTINCT_DEVICES") == "1":
        import torch
        if torch.cuda.device_count() >= n:
            return list(range(n))
    return [0] * n


# every array a BatchEncoding can carry: the nine result arrays of the library (describe() in csrc/capi/sharding.cpp), and the two the
# Python mirror derives from them (the kinds of a mixed batch's inputs, every input's own encoding under overflowing=True)
RESULT_ARRAYS = ("ids", "tok_offsets", "offsets", "word_ids", "type_ids", "seq_ids", "pad_counts", "enc_docs", "enc_parts")
DERIVED_ARRAYS = ("kinds", "_first")


def _equal_batches(a, b, what=""):
    """Two BatchEncoding objects hold the same result: every array is present on both sides or on neither, and equal in dtype, shape
    and content; the counts agree.  (test_the_comparison_covers_every_array_of_a_batch keeps the field list complete.)"""
    assert len(a) == len(b), (what, "len", len(a), len(b))
    assert a.n_tokens == b.n_tokens, (what, "n_tokens", a.n_tokens, b.n_tokens)
    assert a.n_encodings == b.n_encodings, (what, "n_encodings", a.n_encodings, b.n_encodings)
    for f in RESULT_ARRAYS + DERIVED_ARRAYS:
        x, y = getattr(a, f, None), getattr(b, f, None)
        assert (x is None) == (y is None), (what, f, "present on one side only")
        if x is None:
            continue
        assert isinstance(x, np.ndarray) and isinstance(y, np.ndarray), (what, f, type(x), type(y))
        assert x.dtype == y.dtype, (what, f, x.dtype, y.dtype)
        assert x.shape == y.shape, (what, f, x.shape, y.shape)
        if not np.array_equal(x, y):
            k = int(np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))[0])
            raise AssertionError((what, f, "first difference at", k, x[k].tolist(), y[k].tolist()))


def _snapshot(be):
    """an expected result kept across test cases: the arrays copied out of the library's pinned buffers"""
    c = copy.copy(be)
    for k, v in vars(be).items():
        if isinstance(v, np.ndarray):
            setattr(c, k, v.copy())
    return c


def _docs():
    docs = synth.gen_lines(40000, text_seed=301) + ["", "x" * 70000, ""] + synth.stress_lines(seed=45, n=1500) + ["", ""]
    return docs


@pytest.mark.parametrize("collect", ["host", "p2p"])
@pytest.mark.parametrize("n_dev", [2, 3, 5])
def test_sharded_call_equals_the_unsharded_call(collect, n_dev):
    import tokenizers_amd as ta
    js = load_tokenizer_json("bytelevel_prefix_trim_3000")
    one = ta.Tokenizer.from_str(js, device=0)
    many = ta.Tokenizer.from_str(js, device=_devs(n_dev), collect=collect)
    assert many.devices == _devs(n_dev)
    docs = _docs()
    _equal_batches(many.encode_batch_csr(docs), one.encode_batch_csr(docs))
    st = many.shard_stats()
    assert len(st) == n_dev and sum(b for _, b, _ in st) == sum(len(d.encode()) for d in docs) and all(ms > 0 for _, _, ms in st)
    nb = [b for _, b, _ in st]
    assert max(nb) - min(nb) <= 70000 + 200, "byte-balanced shards (one 70 kB document is the granularity here)"
    _equal_batches(many.encode_batch_csr(docs, offsets="char", word_ids=True), one.encode_batch_csr(docs, offsets="char", word_ids=True))
    _equal_batches(many.encode_batch_csr(docs, offsets="byte"), one.encode_batch_csr(docs, offsets="byte"))
    # a batch too small to shard, an empty one, one of empty documents
    for small in (docs[:3], [], ["", "", ""]):
        _equal_batches(many.encode_batch_csr(small), one.encode_batch_csr(small))


def test_sharded_call_vs_oracle_gpt2():
    import tokenizers_amd as ta
    js = synth.load_or_train_gpt2()
    many = ta.Tokenizer.from_str(js, device=_devs(4))
    docs = synth.gen_lines(60000, text_seed=302) + synth.stress_lines(seed=46, n=800)
    exp = orc.Oracle(js).encode_batch(docs)
    got = many.encode_batch_csr(docs)
    assert np.array_equal(got.tok_offsets, exp.tok_offsets) and np.array_equal(got.ids, exp.ids)


@pytest.mark.parametrize("name", ["bert_wordpiece_4000_specials", "llama3_small_6000_specials"])
def test_sharded_pairs_truncation_fixed_padding_and_words(name):
    """what rides on the epilogues: pairs (shards are cut between pairs), truncation, Fixed padding, special tokens, pre-tokenized
    sequences (cut between sequences); BatchLongest padding and the overflowing encodings (both sharded since round 6)"""
    import tokenizers_amd as ta
    d = json.loads(load_tokenizer_json(name))
    d["truncation"] = {"direction": "Right", "max_length": 24, "strategy": "LongestFirst", "stride": 2}
    d["padding"] = {"strategy": {"Fixed": 28}, "direction": "Right", "pad_to_multiple_of": None, "pad_id": 0, "pad_type_id": 0, "pad_token": "[PAD]"}
    js = json.dumps(d)
    one, many = ta.Tokenizer.from_str(js, device=0), ta.Tokenizer.from_str(js, device=_devs(3))
    lines = [l for l in synth.gen_lines(9000, text_seed=303) if "[" not in l]
    pairs = [(a, b) for a, b in zip(lines[0::2], lines[1::2])]
    for kw in ({}, {"offsets": "char", "word_ids": True}):
        _equal_batches(many.encode_batch_csr(lines, add_special_tokens=True, **kw), one.encode_batch_csr(lines, add_special_tokens=True, **kw))
        _equal_batches(many.encode_batch_csr(pairs, add_special_tokens=True, **kw), one.encode_batch_csr(pairs, add_special_tokens=True, **kw))
    words = [l.split(" ") for l in lines]
    _equal_batches(many.encode_batch_csr(words, is_pretokenized=True, add_special_tokens=True), one.encode_batch_csr(words, is_pretokenized=True, add_special_tokens=True))
    # a batch that mixes single sequences and pairs: cut between inputs, every shard with its slice of the inputs' CSR (round 6)
    mixed = [lines[i] if i % 3 else (lines[i], lines[i + 1]) for i in range(0, len(lines) - 1)]
    is_pair = lambda it: isinstance(it, (tuple, list))
    _equal_batches(many._encode_mixed(mixed, "char", True, True, False, False, is_pair), one._encode_mixed(mixed, "char", True, True, False, False, is_pair))
    st = many.shard_stats()
    assert len(st) == 3 and all(nb > 0 for _, nb, _ in st), "the mixed batch went over every device"
    # BatchLongest: sharded since round 6 (the shards exchange their longest encoding); overflowing: the whole batch on devices[0]
    d["padding"]["strategy"] = "BatchLongest"
    js = json.dumps(d)
    one, many = ta.Tokenizer.from_str(js, device=0), ta.Tokenizer.from_str(js, device=_devs(3))
    _equal_batches(many.encode_batch_csr(lines, add_special_tokens=True), one.encode_batch_csr(lines, add_special_tokens=True))
    # overflowing: sharded too since round 6 (a shard knows how many encodings it yields when its kernels are done: the displacements are
    # summed then, its document indices rebased) -- singles and pairs, with the shards' own BatchLongest exchange
    for inp in (lines, pairs):
        a, b = many.encode_batch_csr(inp, add_special_tokens=True, overflowing=True), one.encode_batch_csr(inp, add_special_tokens=True, overflowing=True)
        _equal_batches(a, b)
        assert np.array_equal(a.enc_docs, b.enc_docs) and len(a.enc_docs) > len(inp)
        if a.enc_parts is not None or b.enc_parts is not None:
            assert np.array_equal(a.enc_parts, b.enc_parts)
        st = many.shard_stats()
        assert len(st) == 3 and all(nb > 0 for _, nb, _ in st), "the overflowing batch went over every device"


@pytest.mark.parametrize("n_dev", [2, 3, 5])
def test_batch_longest_padding_is_sharded(n_dev):
    """BatchLongest (utils/padding.rs:55-63) couples the documents of a batch through ONE number, the longest encoding: the shards hand
    theirs to the call's exchange and pad to the batch's -- singles, pairs, pad_to_multiple_of, either side; the longest document sits in
    the LAST shard, so every other shard pads to a length it has not seen.  And a shard that fails must not leave the others waiting."""
    import tokenizers_amd as ta
    d = json.loads(load_tokenizer_json("bert_wordpiece_4000_specials"))
    lines = [l for l in synth.gen_lines(9000, text_seed=305) if "[" not in l]
    lines[-3] = " ".join(lines[:40])                       # the batch's longest, in the last shard
    pairs = [(a, b) for a, b in zip(lines[0::2], lines[1::2])]
    for direction, multiple, trunc in (("Right", None, None), ("Left", 8, None), ("Right", 16, 40)):
        d["padding"] = {"strategy": "BatchLongest", "direction": direction, "pad_to_multiple_of": multiple, "pad_id": 0, "pad_type_id": 0, "pad_token": "[PAD]"}
        d["truncation"] = None if trunc is None else {"direction": "Right", "max_length": trunc, "strategy": "LongestFirst", "stride": 0}
        js = json.dumps(d)
        one, many = ta.Tokenizer.from_str(js, device=0), ta.Tokenizer.from_str(js, device=_devs(n_dev))
        for batch in (lines, pairs):
            got, want = many.encode_batch_csr(batch, add_special_tokens=True, offsets="char", word_ids=True), one.encode_batch_csr(batch, add_special_tokens=True, offsets="char", word_ids=True)
            _equal_batches(got, want)
            lens = np.diff(got.tok_offsets)
            assert lens.min() == lens.max(), "every encoding of the batch has the batch's length"
            st = many.shard_stats()
            if sum(len(x.encode()) for x in lines) >= (n_dev + 1) * 8192:      # (under the CPU emulation the corpus is too small for five shards)
                assert len(st) == n_dev and all(b > 0 for _, b, _ in st), "the call ran on every device of the list"
    # an error in one shard: the call fails, nobody waits for the shard that left, the handle works afterwards
    dw = json.loads(load_tokenizer_json("wordlevel_whitespace_c1"))
    dw["model"]["unk_token"] = "<nope>"           # not in the vocabulary: MissingUnkToken the moment a word misses (wordlevel/mod.rs:175-177)
    dw["padding"] = {"strategy": "BatchLongest", "direction": "Right", "pad_to_multiple_of": None, "pad_id": 0, "pad_type_id": 0, "pad_token": "[PAD]"}
    bad = ta.Tokenizer.from_str(json.dumps(dw), device=_devs(n_dev))
    vocab = [w for w in dw["model"]["vocab"] if w.isascii() and w.isalnum()]
    good = [" ".join(vocab[(7 * i + k) % len(vocab)] for k in range(12)) for i in range(20000)]
    with pytest.raises(Exception, match="MissingUnkToken"):
        bad.encode_batch_csr(good[:-100] + ["zzzzqqqq"] * 100)
    assert bad.encode_batch_csr(good).n_tokens == 12 * len(good)


def test_an_error_in_one_shard_fails_the_call_and_the_handle_survives():
    import tokenizers_amd as ta
    d = json.loads(load_tokenizer_json("wordlevel_whitespace_c1"))
    d["model"]["unk_token"] = "<nope>"            # not in the vocabulary: MissingUnkToken the moment a word misses (wordlevel/mod.rs:175-177)
    many = ta.Tokenizer.from_str(json.dumps(d), device=_devs(3))
    vocab = [w for w in d["model"]["vocab"] if w.isascii() and w.isalnum()]
    good = [" ".join(vocab[(7 * i + k) % len(vocab)] for k in range(12)) for i in range(20000)]
    assert many.encode_batch_csr(good).n_tokens == 12 * len(good)
    bad = list(good)
    bad[len(bad) - 5] = "zzzzunknownzzzz"        # lands in the last shard
    with pytest.raises(Exception, match="MissingUnkToken"):
        many.encode_batch_csr(bad)
    assert many.encode_batch_csr(good).n_tokens == 12 * len(good)


def test_devices_from_the_environment(monkeypatch):
    import tokenizers_amd as ta
    js = load_tokenizer_json("wordlevel_whitespace_c1")
    monkeypatch.setenv("TOKENIZERS_GPU_DEVICES", "0,0")
    assert ta.Tokenizer.from_str(js, device="env").devices == [0, 0]
    monkeypatch.setenv("TOKENIZERS_GPU_DEVICES", "all")
    assert ta.Tokenizer.from_str(js, device="env").devices[0] == 0
    monkeypatch.delenv("TOKENIZERS_GPU_DEVICES")
    assert ta.Tokenizer.from_str(js, device="env").devices == [0]
    monkeypatch.setenv("TOKENIZERS_GPU_DEVICES", "0;1")
    with pytest.raises(ValueError, match="TOKENIZERS_GPU_DEVICES"):
        ta.Tokenizer.from_str(js, device="env")
    with pytest.raises(ValueError, match="named twice"):
        ta.Tokenizer.from_str(js, device=[0, 0], collect="rccl")


def test_rccl_that_cannot_be_opened_falls_back_to_peer_copies():
    """collect="rccl" on a box whose librccl.so cannot be opened (here: TKAMD_RCCL_LIB names a file that is not there) must not fail
    the call, let alone the process (dlerror() returns its message ONCE): the handle says why on stderr, switches to the peer-copy
    collect -- the same bytes over the same links -- and the result is the unsharded call's."""
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, tokenizers_amd as ta\n"
        "from oracle import synth\n"
        "from tests.helpers import load_tokenizer_json\n"
        "js = load_tokenizer_json('bytelevel_prefix_trim_3000')\n"
        "docs = synth.gen_lines(20000, text_seed=305) + ['', 'x' * 30000]\n"
        "one = ta.Tokenizer.from_str(js, device=0).encode_batch_csr(docs, offsets='byte')\n"
        "many = ta.Tokenizer.from_str(js, device=[0, 0, 0], collect='rccl')\n"
        "for _ in range(2):\n"
        "    got = many.encode_batch_csr(docs, offsets='byte')\n"
        "    assert np.array_equal(got.ids, one.ids) and np.array_equal(got.tok_offsets, one.tok_offsets) and np.array_equal(got.offsets, one.offsets)\n"
        "assert len(many.shard_stats()) == 3\n"
        "print('FALLBACK_OK')\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TKAMD_TEST_HOOKS="1", TKAMD_RCCL_LIB="/nonexistent/librccl.so", TKAMD_SHARD_MIN_KB="8"),
                       capture_output=True, text=True, timeout=600)
    assert "FALLBACK_OK" in r.stdout, r.stdout + r.stderr
    assert r.stderr.count("falls back to TKAMD_COLLECT_ROOT_P2P") == 1 and "could not be opened" in r.stderr, r.stderr


@pytest.mark.needs_hw
def test_rccl_collect_on_one_rank():
    """TKAMD_COLLECT_ROOT_RCCL with a one-device list: ncclCommInitAll over [0], rank 0's shard travels through ncclSend / ncclRecv to
    the displacement in the root buffer, then the one D2H."""
    import tokenizers_amd as ta
    js = load_tokenizer_json("bytelevel_prefix_trim_3000")
    one = ta.Tokenizer.from_str(js, device=0)
    docs = _docs()
    want = one.encode_batch_csr(docs, offsets="byte", word_ids=True)
    # (a one-device list has no replicas: the sharded path needs two entries to engage; RCCL refuses a repeated device, so on a
    # one-GPU box the RCCL gather is exercised only where two GPUs exist)
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("RCCL wants one rank per GPU: needs two GPUs")
    many = ta.Tokenizer.from_str(js, device=[0, 1], collect="rccl")
    _equal_batches(many.encode_batch_csr(docs, offsets="byte", word_ids=True), want)
    # the nine-array call: pairs with truncation, padding, char offsets, word ids, special tokens and the overflowing encodings
    js9 = _with_sections("bert_wordpiece_4000_specials", *MATRIX_SECTIONS["bert_wordpiece_4000_specials"])
    pairs = _inputs_of("pairs", _matrix_corpus())
    got = _call(ta.Tokenizer.from_str(js9, device=[0, 1], collect="rccl"), "pairs", pairs)
    assert all(getattr(got, f) is not None for f in RESULT_ARRAYS)
    _equal_batches(got, _call(ta.Tokenizer.from_str(js9, device=0), "pairs", pairs))


@pytest.mark.needs_hw
def test_a_forked_child_fails_cleanly_and_the_parent_goes_on():
    """fork() after the parent initialised HIP (the reference's binding registers a pthread_atfork child handler for the same reason,
    bindings/python/src/lib.rs:41-47): the child's calls on the inherited handle -- and any new device handle -- fail at once with a
    message instead of hanging on the dead runtime; the parent is unaffected."""
    import tokenizers_amd as ta
    js = load_tokenizer_json("wordlevel_whitespace_c1")
    tok = ta.Tokenizer.from_str(js, device=0)
    docs = synth.gen_lines(500, text_seed=304)
    want = tok.encode_batch_csr(docs)
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        msg = b"?"
        try:
            try:
                tok.encode_batch_csr(docs)
                msg = b"encoded"
            except Exception as e:                   # noqa: BLE001
                msg = ("E1:" + str(e)[:60]).encode()
            try:
                ta.Tokenizer.from_str(js, device=0)
                msg += b"|made"
            except Exception as e:                   # noqa: BLE001
                msg += ("|E2:" + str(e)[:60]).encode()
            host_only = ta.Tokenizer.from_str(js, device=-1)
            msg += b"|host-only ok" if host_only.info["vocab_size"] > 0 else b"|host-only bad"
        finally:
            os.write(w, msg)
            os._exit(0)
    os.close(w)
    _, status = os.waitpid(pid, 0)
    out = os.read(r, 4096).decode()
    os.close(r)
    assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == 0, status
    assert out.startswith("E1:this process was fork()ed") and "|E2:this process was fork()ed" in out and out.endswith("host-only ok"), out
    _equal_batches(tok.encode_batch_csr(docs), want)


# ---- every result array of a sharded call, in every collect mode ----
# Handles and expected results are kept from one parametrised case to the next (the cases are ordered tokenizer first): under the CPU
# emulation a handle takes seconds to load, and the unsharded result of one batch serves every device list and collect mode.
_IS_PAIR = lambda it: isinstance(it, (tuple, list))          # noqa: E731
_COLLECT = {"host": 0, "p2p": 1}
_many_kept: dict = {}
_one_kept: dict = {}
_expected: dict = {}


def _one(js):
    import tokenizers_amd as ta
    if js not in _one_kept:
        while len(_one_kept) >= 2:                           # (two at a time: a cut test runs two section rows of one tokenizer)
            old = next(iter(_one_kept))
            del _one_kept[old]
            for key in [k for k in _expected if k[0] == old]:
                del _expected[key]
        _one_kept[js] = ta.Tokenizer.from_str(js, device=0)
    return _one_kept[js]


def _many(js, n_dev, collect):
    """the n_dev-device handle of a tokenizer.json (two kept at a time), in the collect mode asked for: made with it, or switched to
    it the way the constructor sets it (tkamd_tokenizer_set_collect of the C ABI).  The cases are ordered host before p2p, so a p2p
    row usually runs on a handle that was made as "host" and has no root buffer yet: its first peer-copy call grows the handle's
    buffers to the call's descriptors, which is the path under test; later p2p calls with fewer or more arrays reuse and extend them."""
    import tokenizers_amd as ta
    from tokenizers_amd import _lib
    key = (js, n_dev, os.environ.get("TKAMD_SHARD_MIN_KB"))
    if key not in _many_kept:
        while len(_many_kept) >= 2:
            del _many_kept[next(iter(_many_kept))]
        _many_kept[key] = ta.Tokenizer.from_str(js, device=_devs(n_dev), collect=collect)
    many = _many_kept[key]
    assert many.devices == _devs(n_dev)
    if many._collect != collect:
        _lib.check(many._lib.tkamd_tokenizer_set_collect(many._h, {"host": _lib.COLLECT_HOST, "p2p": _lib.COLLECT_ROOT_P2P}[collect]))
        many._collect = collect
    return many


def _with_sections(name, trunc_direction, pad_strategy, multiple=None, pad_direction="Right"):
    d = json.loads(load_tokenizer_json(name))
    d["truncation"] = {"direction": trunc_direction, "max_length": 24, "strategy": "LongestFirst", "stride": 2}
    d["padding"] = None if pad_strategy is None else {"strategy": pad_strategy, "direction": pad_direction, "pad_to_multiple_of": multiple, "pad_id": 0,
                                                      "pad_type_id": 0, "pad_token": "[PAD]"}
    return json.dumps(d)


def _call(tok, kind, inputs, offsets="char", special=True, overflowing=True):
    if kind == "mixed":
        return tok._encode_mixed(inputs, offsets, True, special, False, overflowing, _IS_PAIR)
    return tok.encode_batch_csr(inputs, offsets=offsets, word_ids=True, add_special_tokens=special, is_pretokenized=kind == "words", overflowing=overflowing)


def _n_bytes(inputs) -> int:
    return sum(len(x.encode()) if isinstance(x, str) else _n_bytes(x) for x in inputs)


def _sharded(many, n_dev, inputs, call, what):
    """the call's result, after checking on shard_stats() that THIS call was cut over the n_dev devices (the statistics are those of the
    last sharded call: a call that ran on devices[0] alone leaves the previous ones, busy times included, in place)"""
    before = many.shard_stats()
    got = call(many)
    st = many.shard_stats()
    assert len(st) == n_dev and st != before, (what, "the call was not sharded", st)
    assert sum(b for _, b, _ in st) == _n_bytes(inputs), (what, st)
    return got, [b for _, b, _ in st]


def _want(js, label, call):
    """the unsharded handle's result of `call`, kept under the tokenizer.json, the case's label and the size regime of the corpora"""
    one = _one(js)
    key = (js, label, synth.gen_lines, os.environ.get("TKAMD_SIMT"))
    if key not in _expected:
        _expected[key] = _snapshot(call(one))
    return _expected[key]


_corpora: dict = {}


def _kept(make, *key):
    """a corpus made once per process and size regime (the CPU suite's slice shrinks oracle.synth itself)"""
    key = key + (synth.gen_lines, os.environ.get("TKAMD_SIMT"))
    if key not in _corpora:
        _corpora[key] = make()
    return _corpora[key]


def _lines(n, seed):
    """synthetic lines without '[' (the one filter the sharded tests apply): at least 95 % of the lines survive it"""
    def make():
        raw = synth.gen_lines(n, text_seed=seed)
        kept = [l for l in raw if "[" not in l]
        assert len(kept) >= 0.95 * len(raw), (len(kept), len(raw))
        return kept
    return _kept(make, "lines", n, seed)


def _matrix_corpus():
    """lines, the adversarial set, empty documents, one document longer than the smallest shard -- about 3 MB (30 kB under the CPU
    emulation: oracle.synth hands out 300 lines at least there, of which a part is taken)"""
    def make():
        raw = synth.gen_lines(N(24000), text_seed=311)[:N(24000, floor=150)] + synth.stress_lines(seed=47, n=N(1500, floor=150))[:N(1500, floor=70)]
        kept = [l for l in raw if "[" not in l]
        assert len(kept) >= 0.95 * len(raw), (len(kept), len(raw))
        third = len(kept) // 3
        return kept[:third] + ["", "x y" * (N(70000, floor=6000) // 3), ""] + kept[third:2 * third] + ["", ""] + kept[2 * third:]
    return _kept(make, "matrix")


def _inputs_of(kind, docs):
    if kind == "singles":
        return docs
    if kind == "pairs":
        return list(zip(docs[0::2], docs[1::2]))
    if kind == "mixed":
        return [docs[i] if i % 3 else (docs[i], docs[i + 1]) for i in range(len(docs) - 1)]
    return [d.split(" ") for d in docs]                  # words: runs of spaces leave empty words, an empty document one empty word


# tokenizer -> (truncation direction, padding strategy, pad_to_multiple_of, padding direction); every fixture here has a pair layout
# (a template, BertProcessing, the ByteLevel processor, or no post-processor at all), so every row takes all four kinds of input
MATRIX_SECTIONS = {
    "bytelevel_prefix_trim_3000": ("Right", {"Fixed": 28}, None, "Right"),
    "bert_wordpiece_4000_specials": ("Right", "BatchLongest", 8, "Right"),
    "llama3_small_6000_specials": ("Left", {"Fixed": 28}, None, "Right"),
    "spm_bpe_llama2": ("Right", "BatchLongest", 8, "Left"),
    "spm_bpe_split": ("Right", {"Fixed": 28}, None, "Left"),
    "bpe_ws_byte_fallback": ("Left", "BatchLongest", 8, "Right"),
}
MATRIX_KINDS = ("singles", "pairs", "mixed", "words")
MATRIX = [pytest.param(name, n_dev, collect, kind, id="%s-%ddev-%s-%s" % (name, n_dev, collect, kind))
          for name in MATRIX_SECTIONS for n_dev in (2, 3, 5) for collect in ("host", "p2p") for kind in MATRIX_KINDS]


def check_matrix_case(monkeypatch, name, n_dev, collect, kind):
    monkeypatch.setenv("TKAMD_SHARD_MIN_KB", "4")            # (read when a handle is made) five shards out of the emulation's 30 kB
    js = _with_sections(name, *MATRIX_SECTIONS[name])
    inputs = _inputs_of(kind, _matrix_corpus())
    many = _many(js, n_dev, collect)
    requests = [("char", lambda t: _call(t, kind, inputs))]
    if kind == "singles":                                    # byte offsets: once per tokenizer, device list and collect mode
        requests.append(("byte", lambda t: _call(t, kind, inputs, offsets="byte")))
    for label, call in requests:
        what = (name, n_dev, collect, kind, label)
        got, nb = _sharded(many, n_dev, inputs, call, what)
        if kind in ("pairs", "mixed"):
            assert all(getattr(got, f) is not None for f in RESULT_ARRAYS), (what, "not the nine-array call")
        assert got.n_encodings > len(inputs), (what, "no overflowing encodings")
        _equal_batches(got, _want(js, (kind, label), call), what)
        assert all(b > 0 for b in nb), (what, "a device without bytes", nb)


@pytest.mark.parametrize("name,n_dev,collect,kind", MATRIX)
def test_every_array_of_a_sharded_call(monkeypatch, name, n_dev, collect, kind):
    """Tokenizer family x input kind x collect mode x device count, every one with a truncation and a padding section and the full
    request -- char offsets, word ids, special tokens, overflowing encodings: six result arrays for single and pre-tokenized
    sequences, all nine for pairs and mixed batches (the call Tokenizer.encode_batch makes) -- against the unsharded handle's result."""
    check_matrix_case(monkeypatch, name, n_dev, collect, kind)


def test_the_comparison_covers_every_array_of_a_batch():
    """_equal_batches walks a fixed list of fields: a BatchEncoding of the nine-array call carries no array outside that list (an array
    added to the result later is either compared or named here), and all nine of the library's."""
    js = _with_sections("bert_wordpiece_4000_specials", "Right", {"Fixed": 28})
    lines = _lines(N(2000), 313)
    be = _call(_one(js), "pairs", list(zip(lines[0::2], lines[1::2])))
    carried = {k for k, v in vars(be).items() if isinstance(v, np.ndarray)}
    assert carried <= set(RESULT_ARRAYS + DERIVED_ARRAYS), carried - set(RESULT_ARRAYS + DERIVED_ARRAYS)
    assert set(RESULT_ARRAYS) <= carried, set(RESULT_ARRAYS) - carried
    _equal_batches(be, _snapshot(be))
    for f in RESULT_ARRAYS:                                  # ... and a difference in any one of them is seen
        other = _snapshot(be)
        getattr(other, f).reshape(-1)[-1] ^= 1
        with pytest.raises(AssertionError):
            _equal_batches(be, other)
        if f not in ("ids", "tok_offsets"):                  # (the two every batch has)
            setattr(other, f, None)
            with pytest.raises(AssertionError):
                _equal_batches(be, other)


# ---- the cuts ----
CUT_SECTIONS = {
    "bert-batchlongest": ("bert_wordpiece_4000_specials", ("Right", "BatchLongest", 8), True),
    "bert-nopadding-nospecials": ("bert_wordpiece_4000_specials", ("Left", None), False),       # whitespace documents yield no token at all
    "spm_llama2-fixed": ("spm_bpe_llama2", ("Right", {"Fixed": 28}, None, "Left"), True),           # (the CPU suite's slice; the matrix above runs this family)
}


def _text(n_bytes, k):
    """dense text of about n_bytes bytes, different for every k"""
    pool = _kept(lambda: " ".join(_lines(N(400), 314)), "pool")
    lo = (k * 1777) % (len(pool) // 2)
    return (pool[lo:] + " " + pool)[:n_bytes].strip()


def _cut_cases(kind, n_dev):
    """label -> (inputs, a shard without documents is certain, the inputs depend on n_dev).  The short documents on either side of the
    long one hold less than a fifth of a shard's share, so all n_dev - 1 byte targets fall inside it and every cut lands on one of its two ends: of the shards between two such cuts at most one holds it and
    the others hold nothing.  That leaves an empty shard for any device count when the document is alone, from three devices on
    when it is the first or the last, from four on when short documents sit on both sides."""
    # (TKAMD_SHARD_MIN_KB=1 wants n_dev kB in a batch: under the emulation the sizes are what that takes, pre-tokenized -- the
    # spaces gone -- included)
    L, K = N(40000, floor=8000), N(4000, floor=1600)
    long_doc, short = _text(L, 0), [_text(40 + 7 * i, i + 1) for i in range(4)]
    tiny = ["a", "b c", "", "d"]
    ws = "\t\n \r\n\t" * (K // 24)                               # a document of whitespace only
    few = [_text(N(4000, floor=1500 * n_dev // (n_dev - 1)), 10 + i) for i in range(n_dev - 1)]
    seven = [_text(K + 61 * i, 20 + i) for i in range(7)]           # 7 inputs of about equal size: no byte target of 2, 3 or 5 devices on a boundary
    groups = [[_text(K // 2, 40 + 2 * g), _text(K // 2, 41 + 2 * g)] for g in range(n_dev)]
    empties = [""] * (2 * n_dev)                                # as many documents as a shard's share of this batch
    runs = [d for g in groups for d in g + empties][:-len(empties)]
    same = [d for g in groups for d in [groups[0][0]] * 2 + empties]          # equal groups: every byte target on the first empty document of a run
    singles = {
        "long alone": ([long_doc], True),
        "long first": ([long_doc] + short, n_dev >= 3),
        "long between": (short[:2] + [long_doc] + short[2:], n_dev >= 4),
        "long last": (short + [long_doc], n_dev >= 3),
        "fewer inputs than devices": (few, False),
        "targets inside inputs": (seven, False),
        "runs of empty documents": (runs, False),
        "runs of empty documents on the targets": (same, False),
        "no tokens in the first shards": ([ws] * 12 + [_text(K // 4, 60 + i) for i in range(12)], False),
        "no tokens in the last shards": ([_text(K // 4, 70 + i) for i in range(12)] + [ws] * 12, False),
    }
    per_dev = ("fewer inputs than devices", "runs of empty documents", "runs of empty documents on the targets")
    singles = {label: (docs, zero, label in per_dev) for label, (docs, zero) in singles.items()}
    if kind == "singles":
        return singles
    both = ("targets inside inputs",)                        # this one in both orders, the others alternately
    if kind == "pairs":
        # one side tiny, the other the document: the byte target falls in the first or in the second sequence of a pair
        out = {}
        for k, (label, (docs, zero, dep)) in enumerate(singles.items()):
            if k % 2 == 0 or label in both:
                out[label + " (tiny, doc)"] = ([(tiny[i % 4], d) for i, d in enumerate(docs)], zero, dep)
            if k % 2 == 1 or label in both:
                out[label + " (doc, tiny)"] = ([(d, tiny[i % 4]) for i, d in enumerate(docs)], zero, dep)
        return out
    if kind == "mixed":
        out = {}
        for k, (label, (docs, zero, dep)) in enumerate(singles.items()):
            if k % 2 == 0 or label in both:
                out[label] = ([d if i % 3 == 0 else ((tiny[i % 4], d) if i % 3 == 1 else (d, tiny[i % 4])) for i, d in enumerate(docs)], zero, dep)
            if k % 2 == 1 or label in both:
                out[label + ", pairs first"] = ([d if i % 3 == 2 else ((d, tiny[i % 4]) if i % 3 == 1 else (tiny[i % 4], d)) for i, d in enumerate(docs)], zero, dep)
        return out
    # pre-tokenized: a document becomes a sequence of words (with empty words where two spaces met), an empty document an empty
    # SEQUENCE (no word at all) or a sequence of one empty word, alternately
    out = {}
    for label, (docs, zero, dep) in singles.items():
        seqs = [(d.replace("e ", "e  ").split(" ") if d else ([] if i % 2 else [""])) for i, d in enumerate(docs)]
        out[label] = (seqs, zero, dep)
    return out


CUTS = [pytest.param(n_dev, overflowing, collect, id="%ddev-%s-%s" % (n_dev, "overflowing" if overflowing else "plain", collect))
        for n_dev in (2, 3, 5) for overflowing in (False, True) for collect in ("host", "p2p")]
# without padding and special tokens a whitespace document yields no token at all: the cases that put such shards in front of and
# behind dense text, and one with shards that hold no document (every other case runs with BatchLongest padding and special tokens)
NO_TOKEN_CASES = ("no tokens in the first shards", "no tokens in the last shards", "long between")


def check_cuts(monkeypatch, cfg, n_dev, overflowing, collect, kinds=MATRIX_KINDS, only=None):
    monkeypatch.setenv("TKAMD_SHARD_MIN_KB", "1")            # (read when a handle is made) the smallest the library takes
    name, sections, special = CUT_SECTIONS[cfg]
    js = _with_sections(name, *sections)
    many = _many(js, n_dev, collect)
    n_zero = 0
    for kind in kinds:
        for label, (inputs, zero, per_dev) in _cut_cases(kind, n_dev).items():
            if only is not None and not label.startswith(only):
                continue
            what = (cfg, n_dev, overflowing, collect, kind, label)
            call = lambda t: _call(t, kind, inputs, special=special, overflowing=overflowing)      # noqa: E731
            got, nb = _sharded(many, n_dev, inputs, call, what)
            if zero:
                assert min(nb) == 0, (what, "no device without bytes", nb)
                n_zero += 1
            _equal_batches(got, _want(js, (n_dev if per_dev else 0, overflowing, kind, label), call), what)
    return n_zero


@pytest.mark.parametrize("n_dev,overflowing,collect", CUTS)
def test_the_cuts_of_a_sharded_call(monkeypatch, n_dev, overflowing, collect):
    """Shards of a few hundred bytes (TKAMD_SHARD_MIN_KB=1): shards without a document in front of, between and behind the others,
    fewer inputs than devices, byte targets inside a pair / a mixed input / a pre-tokenized sequence, empty documents, empty words and
    empty sequences on the cuts, shards that yield no token in front of and behind dense text.  Every call is seen to be sharded."""
    n_zero = check_cuts(monkeypatch, "bert-batchlongest", n_dev, overflowing, collect)
    assert n_zero >= len(MATRIX_KINDS), "the cases with a shard without documents ran"
    check_cuts(monkeypatch, "bert-nopadding-nospecials", n_dev, overflowing, collect, only=NO_TOKEN_CASES)


# ---- against the reference ----
@pytest.mark.parametrize("name", ["bert_wordpiece_4000_specials", "llama3_small_6000_specials", "spm_bpe_llama2"])
def test_sharded_encode_batch_matches_the_reference(name, ref_tokenizers):
    """What a user calls: Tokenizer.encode_batch on a three-device handle (peer-copy collect) against the reference's encode_batch of
    the same tokenizer.json -- single sequences, pairs and a batch that mixes them; every field of every encoding and of every entry
    of its `overflowing`."""
    js = _with_sections(name, *MATRIX_SECTIONS[name])
    ref, many = ref_tokenizers.Tokenizer.from_str(js), _many(js, 3, "p2p")
    docs = _lines(N(3000), 315) + ["", "x y" * (N(30000, floor=6000) // 3), ""] + _lines(N(1500), 316)[:N(1500, floor=20)]
    fields = lambda e: (e.ids, e.type_ids, e.tokens, [tuple(o) for o in e.offsets], e.word_ids, e.attention_mask, e.special_tokens_mask, e.sequence_ids)   # noqa: E731
    deep = lambda e: [fields(e)] + [fields(o) for o in e.overflowing]                          # noqa: E731
    for kind in ("singles", "pairs", "mixed"):
        inputs = _inputs_of(kind, docs)
        got, nb = _sharded(many, 3, inputs, lambda t: t.encode_batch(inputs), (name, kind))
        assert all(b > 0 for b in nb), (name, kind, nb)
        exp = ref.encode_batch(inputs)
        assert len(got) == len(exp) == len(inputs)
        n_over = 0
        for i, e in enumerate(exp):
            assert deep(got[i]) == deep(e), (name, kind, i, inputs[i])
            n_over += len(e.overflowing)
        assert n_over > 0, "the truncation left overflowing encodings"
