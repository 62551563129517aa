"""-m gpu: the FUSED streaming decode (tkamd_decode_stream_new with TKAMD_STREAM_FUSED, Tokenizer.decode_stream(fused=True): one kernel
with a lane per stream in front of the scan and the copy, no host wait, buffers sized by a bound) against the restatement of the
reference's step_decode_stream (tests/decode_stream_ref.py IntStream), as tests/test_decode_stream_gpu.py holds the unfused step to it: at
every step the status and the chunk bytes of every stream and the contract of the text -- here with n_bytes == -1 on the host, the count
on the device, a monotone CSR from 0 to it and the zero slack behind it --, and behind the last step the window state of every stream.
Raw pointers, so everything but the graph capture runs under the SIMT emulation as well."""
import numpy as np
import pytest

from oracle.decode_oracle import DecodeOracle
from tests import decode_cases as dc
from tests import decode_stream_ref as dsr
from tests.test_decode_stream_gpu import N_STEPS, PAD, Pair, _byte_level_case, _case_named, _loaded, _spread, _up

pytestmark = pytest.mark.gpu


def _llama2_case():
    return _case_named("spm_bpe_llama2")


class FusedPair(Pair):
    """Pair over a fused object: the same steps and the same comparison, the text's contract as a fused step states it"""

    def __init__(self, case, n, skip, window=32, label=""):
        super().__init__(case, n, skip, window, label)
        self.ds = self.tk.decode_stream(n, skip_special_tokens=skip, window=window, fused=True)
        assert self.ds.fused is True

    def check(self, text, ids, active=None):
        where = f"{self.label} fused skip={self.skip} step {self.steps}"
        assert text.n_bytes == -1, where                       # the host does not hold the count
        n_bytes = text.n_bytes_device()
        assert 0 <= n_bytes <= self.ds.chunk_capacity, (where, n_bytes)
        raw, off, status = self.ds.read(text, slack=PAD)
        raw, off = raw.tobytes(), [int(x) for x in off]
        assert text.n_docs == self.n and len(off) == self.n + 1 and len(raw) == n_bytes + PAD, where
        assert off[0] == 0 and off[-1] == n_bytes, (where, off[:3], off[-1], n_bytes)
        assert all(a <= b for a, b in zip(off[:-1], off[1:])), where
        assert raw[n_bytes:] == b"\0" * PAD, where
        got = [(int(status[i]), raw[off[i]:off[i + 1]]) for i in range(self.n)]
        exp = [self.refs[i].step(ids[i]) if active is None or active[i] else (dsr.INACTIVE, b"") for i in range(self.n)]
        bad = [(i, got[i], exp[i]) for i in range(self.n) if got[i] != exp[i]]
        assert not bad, f"{where}: {len(bad)} of {self.n} streams differ, first (stream, got, expected) {bad[0]!r}"
        for s, c in got:
            self.seen[s] += 1
            c.decode("utf-8")                                  # strict: a chunk is valid UTF-8
        self.steps += 1
        return got


def test_the_getter_and_the_flag():
    """what tells a fused object from one that only ignored the flag: the getter, the capacities, the keyword"""
    case = _byte_level_case()
    tk, _ = _loaded(case)
    plain, fused = tk.decode_stream(5, window=8), tk.decode_stream(5, window=8, fused=True)
    assert (plain.fused, plain.chunk_capacity, plain.scratch_bytes) == (False, 0, 0)
    assert fused.fused is True and fused.chunk_capacity > 0 and fused.scratch_bytes == 4 * fused.chunk_capacity     # (ByteLevel: 4 strings a stream)
    assert fused.chunk_capacity % (5 * 16) == 0 and fused.chunk_capacity >= 5 * 8 * 3
    chain = _loaded(_llama2_case())[0].decode_stream(3, window=8, fused=True)
    assert chain.scratch_bytes == 3 * chain.chunk_capacity
    empty = tk.decode_stream(0, fused=True)
    assert (empty.fused, empty.chunk_capacity) == (True, 0)


@pytest.mark.parametrize("k", range(len(dc.DECODERS)), ids=dc.case_id)
def test_fused_streams_vs_restatement(k):
    """Every decoder case: its sequences as parallel streams, both skip values, 48 steps, window 64"""
    case = dc.Case(k)
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(500 + k), N_STEPS)]
    seen = [0] * 5
    for skip in (True, False):
        p = FusedPair(case, len(seqs), skip, window=64, label=dc.case_id(k))
        p.run(seqs)
        seen = [a + b for a, b in zip(seen, p.seen)]
    assert seen[dsr.CHUNK] > 0 and seen[dsr.INACTIVE] == 0 and seen[dsr.WINDOW_FULL] == 0, seen


@pytest.mark.parametrize("which", ["bytelevel", "llama2"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_fused_stream_counts_at_lane_wavefront_and_workgroup_edges(n, which):
    case = _byte_level_case() if which == "bytelevel" else _llama2_case()
    base = [q for _, q in dsr.sequences(case, dc.rng_for(901), N_STEPS)]
    n_steps = 48 if n <= 65 else 12
    p = FusedPair(case, n, True, label=f"{n} streams {which}")
    p.run(_spread(base, n, n_steps), n_steps)
    if n:
        assert p.seen[dsr.CHUNK] and p.seen[dsr.NOTHING], p.seen
    else:
        assert p.steps == n_steps


def test_fused_active_mask_that_changes_every_step():
    case = _case_named("bpe_ws_byte_fallback", dc.DECODERS[7][1])
    base = [q for _, q in dsr.sequences(case, dc.rng_for(902), N_STEPS)]
    n = 70
    rng = dc.rng_for(903)
    masks = rng.integers(0, 2, size=(N_STEPS, n)).astype(np.uint8)
    masks[:, 5] = 0                                            # never stepped
    masks[:, 6] = 1
    masks[3] = masks[17] = masks[18] = 0                       # nobody steps
    masks[:4, 66] = 0
    p = FusedPair(case, n, False, label="mask")
    p.run(_spread(base, n, N_STEPS), N_STEPS, active=lambda j: masks[j])
    assert p.seen[dsr.INACTIVE] == int((masks == 0).sum()) and p.seen[dsr.CHUNK] and p.ds.peek(5) == ([], 0, 0)


def test_fused_full_window_sticks_one_stream_until_it_alone_is_reset():
    case = _byte_level_case()
    sp, w = case.specials[0], case.words
    p = FusedPair(case, 3, True, window=4, label="window=4")
    for j in range(4):                                         # five skipped specials in a row on stream 1
        assert p.step([w[10 + j], sp, w[20 + j]])[1] == (dsr.NOTHING, b"")
    assert p.step([w[15], sp, w[25]])[1] == (dsr.WINDOW_FULL, b"")
    got = p.step([w[16], w[30], w[26]])                        # an id that would fit an emptier window: still stuck
    assert got[1] == (dsr.WINDOW_FULL, b"") and got[0][0] == got[2][0] == dsr.CHUNK
    p.check_state()
    assert p.ds.peek(1)[0] == [sp] * 4
    p.ds.reset([1])
    p.refs[1].reset()
    got = p.step([w[17], w[31], w[27]])
    assert [s for s, _ in got] == [dsr.CHUNK] * 3 and got[1][1] == p.decode([w[31]], True)
    p.check_state()


def test_fused_window_of_two():
    case = _byte_level_case()
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(904), N_STEPS)]
    p = FusedPair(case, len(seqs), False, window=2, label="window=2")
    p.run(seqs)
    assert p.seen[dsr.CHUNK] and p.seen[dsr.WINDOW_FULL], p.seen
    p.ds.reset()                                               # everybody steps again behind a reset of all
    for r in p.refs:
        r.reset()
    p.run(seqs, 6)


def test_fused_seed_then_steps():
    case = _case_named("bpe_ws_byte_fallback", dc.DECODERS[7][1])
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(906), N_STEPS)]
    p = FusedPair(case, len(seqs), True, window=8, label="seed")
    for i, q in enumerate(seqs):
        k = i % 4                                              # (0: a seed of nothing is a reset)
        p.ds.seed(i, q[:k])
        p.refs[i].seed(q[:k])
    p.check_state()
    p.run([q[i % 4:] + q for i, q in enumerate(seqs)], 24)
    p.ds.seed(1, seqs[1][:8])                                  # a full window from the start: the next step cannot push
    p.refs[1].seed(seqs[1][:8])
    assert p.step([q[0] for q in seqs])[1] == (dsr.WINDOW_FULL, b"")
    p.check_state()


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_fused_id_types_and_values_that_are_no_id(dtype):
    case = _byte_level_case()
    seqs = [list(q) for _, q in dsr.sequences(case, dc.rng_for(907), N_STEPS)]
    for i, q in enumerate(seqs):
        for j in range(i % 5, N_STEPS, 5):
            q[j] = (-1, -100, case.n_ids + 7)[(i + j) % 3]
            if dtype == "int64" and (i + j) % 4 == 0:
                q[j] = (2 ** 32, 2 ** 40, -2 ** 63, 2 ** 63 - 1)[(i + j) % 4]
    if dtype == "int64":
        seqs[0][1] = 2 ** 32
    p = FusedPair(case, len(seqs), True, label=dtype)
    for j in range(N_STEPS):
        p.step([q[j] for q in seqs], dtype=dtype)
    assert p.seen[dsr.CHUNK] and p.seen[dsr.NOTHING]
    p.check_state()


def _longest(case, decode):
    """(id, bytes) of the id whose decode on its own is the longest"""
    best = max(sorted(case.id2tok), key=lambda i: len(decode([i], False)))
    return best, decode([best], False)


@pytest.mark.parametrize("which", ["bytelevel", "llama2"])
def test_a_window_of_the_longest_token_reaches_the_bound_exactly(which):
    """window ids of the longest token in every stream: the step's string is window x L bytes -- the whole of the place the bound gives
    it -- and the text's zero slack still stands behind the chunks"""
    case = _byte_level_case() if which == "bytelevel" else _llama2_case()
    tk, decode = _loaded(case)
    big, one = _longest(case, decode)
    window, n = 4, 3
    whole = decode([big] * window, False)
    L = len(whole) // window
    assert len(one) >= 3 and L >= len(one) - 1                 # (a first-position form may be a byte shorter)
    p = FusedPair(case, n, False, window=window, label="longest " + which)
    cap = -(-window * max(len(one), 3) // 16) * 16
    assert p.ds.chunk_capacity == n * cap, (p.ds.chunk_capacity, n, cap, len(one))
    for i in range(n):
        p.ds.seed(i, [big] * (window - 1))
        p.refs[i].seed([big] * (window - 1))
    got = p.step([big] * n)                                    # n0 = window - 1 ids become the prefix, the window is full with this id
    assert [s for s, _ in got] == [dsr.CHUNK] * n and all(len(c) == len(whole) - len(decode([big] * (window - 1), False)) for _, c in got)
    p.check_state()
    got = p.step([big] * n)
    assert [s for s, _ in got] == [dsr.CHUNK] * n
    p.check_state()


def test_fused_and_unfused_objects_of_one_handle_in_turn():
    """the same ids into a fused and an unfused object of one handle, a decode_batch_device call between two steps: bytes, status and
    state identical at every step"""
    case = _byte_level_case()
    tk, decode = _loaded(case)
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(908), N_STEPS)]
    n = len(seqs)
    f, u = tk.decode_stream(n, skip_special_tokens=True, window=8, fused=True), tk.decode_stream(n, skip_special_tokens=True, window=8)
    o = DecodeOracle(case.json)
    flat = [i for q in seqs for i in q]
    keep = [_up(np.asarray(flat, dtype=np.uint32)), _up(np.arange(0, len(flat), N_STEPS, dtype=np.int64)),
            _up(np.arange(N_STEPS, len(flat) + 1, N_STEPS, dtype=np.int64))]
    whole = [o.decode(q, True) for q in seqs]
    statuses = set()
    for j in range(N_STEPS):
        kept = _up(np.asarray([q[j] for q in seqs], dtype=np.uint32))
        tf, _ = f.step_device(kept[1], 0, "uint32")
        other = tk.decode_batch_device(keep[0][1], len(flat), keep[1][1], keep[2][1], n, skip_special_tokens=True)
        tu, _ = u.step_device(kept[1], 0, "uint32")
        assert tf.n_bytes == -1 and tu.n_bytes >= 0
        assert other.to_strings() == whole
        rf, ru = f.read(tf, slack=PAD), u.read(tu, slack=PAD)
        assert tf.n_bytes_device() == tu.n_bytes
        for a, b in zip(rf, ru):
            assert a.tobytes() == b.tobytes(), f"step {j}"
        assert [f.peek(i) for i in range(n)] == [u.peek(i) for i in range(n)], f"step {j}"
        statuses.update(int(x) for x in rf[2])
    assert {dsr.NOTHING, dsr.CHUNK} <= statuses


def test_fused_host_step_returns_strings():
    import tokenizers_amd as ta
    case = _byte_level_case()
    tk, decode = _loaded(case)
    sp, w = case.specials[0], case.words
    ds = tk.decode_stream(4, skip_special_tokens=True, window=2, fused=True)
    refs = [dsr.IntStream(decode, True, 2) for _ in range(4)]

    def expect(ids, active=None):
        out = [refs[i].step(ids[i]) if active is None or active[i] else (2, b"") for i in range(4)]
        return [s for s, _ in out], [c.decode() if s == 1 else None for s, c in out]

    for ids, active in (([w[50], sp, w[51], w[52]], None), (np.array([w[53], sp, w[54], w[55]], dtype=np.int64), [1, 1, 0, 1])):
        status, chunks = expect(list(ids), active)
        assert max(status) < 3 and ds.step(ids, active) == chunks
    ids = [w[56], sp, w[57], w[58]]                            # the third special does not fit stream 1's window of two
    status, chunks = expect(ids)
    with pytest.raises(ta.DecodeStreamError, match="stream 1: window full") as e:
        ds.step(ids)
    assert e.value.status == status and e.value.chunks == chunks


def test_a_fused_object_beyond_the_limit_is_refused_by_name():
    case = _byte_level_case()
    tk, _ = _loaded(case)
    with pytest.raises(ValueError, match=r"n_streams = 100000, window = 1024 and L = \d+"):      # (10^8 slots x 3 bytes x 5 > 1 GiB whatever L is)
        tk.decode_stream(100_000, window=1024, fused=True)
    assert tk.decode_stream(2, fused=True).step([case.words[3]] * 2) == [tk.decode([case.words[3]])] * 2


@pytest.mark.needs_hw
@pytest.mark.parametrize("which", ["bytelevel", "llama2"])
def test_one_fused_step_captured_in_a_graph_and_replayed(which):
    """65 streams; one step_tensor captured in a torch.cuda.CUDAGraph behind a warm-up step, 48 replays with new ids copied into the
    static tensor, every replay held against the restatement"""
    import torch
    case = _byte_level_case() if which == "bytelevel" else _llama2_case()
    tk, decode = _loaded(case)
    n = 65
    base = [q for _, q in dsr.sequences(case, dc.rng_for(912), N_STEPS)]
    seqs = _spread(base + base, n, N_STEPS + 1)
    ds = tk.decode_stream(n, skip_special_tokens=True, fused=True)
    refs = [dsr.IntStream(decode, True) for _ in range(n)]
    static_ids = torch.zeros(n, dtype=torch.int64, device="cuda")

    def feed(j):
        static_ids.copy_(torch.tensor([q[j] for q in seqs], dtype=torch.int64), non_blocking=False)
        return [refs[i].step(seqs[i][j]) for i in range(n)]

    side = torch.cuda.Stream()
    exp = feed(0)
    with torch.cuda.stream(side):                              # the warm-up step, outside the capture, on the stream that will capture
        text, status = ds.step_tensor(static_ids)
    side.synchronize()
    assert status.cpu().tolist() == [s for s, _ in exp] and text.to_strings() == [c.decode() for _, c in exp]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        text, status = ds.step_tensor(static_ids)
    assert text.n_bytes == -1
    seen = set()
    for j in range(1, N_STEPS + 1):
        exp = feed(j)
        graph.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [s for s, _ in exp], f"replay {j}"
        n_bytes = int(text.n_bytes_tensor().cpu()[0])
        off = text.doc_offsets_tensor().cpu().tolist()
        raw = text._tensor(text.bytes_ptr, (n_bytes + PAD,), "|u1").cpu().numpy().tobytes()
        assert off[0] == 0 and off[-1] == n_bytes == sum(len(c) for _, c in exp) and raw[n_bytes:] == b"\0" * PAD, f"replay {j}"
        assert [raw[off[i]:off[i + 1]] for i in range(n)] == [c for _, c in exp], f"replay {j}"
        seen.update(s for s, _ in exp)
    assert {dsr.NOTHING, dsr.CHUNK} <= seen
    for i, r in enumerate(refs):
        assert ds.peek(i) == r.state()
