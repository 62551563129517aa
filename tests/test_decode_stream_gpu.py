"""-m gpu: streaming decode on the device (tkamd_decode_stream_*: DecodeStream for a batch of running sequences) against the restatement of
the reference's step_decode_stream (tests/decode_stream_ref.py IntStream, which tests/test_decode_stream_ref.py holds to the wheel's
DecodeStream on these very sequences): at every step the status and the chunk bytes of every stream and the contract of the text (a
monotone CSR that ends at n_bytes, the count on the device, the zero slack), and behind the last step the window state of every stream.
Raw pointers as in tests/test_decode_device_gpu.py, so everything but step_tensor runs under the SIMT emulation as well."""
import os

import numpy as np
import pytest

from oracle.decode_oracle import DecodeOracle
from tests import decode_cases as dc
from tests import decode_stream_ref as dsr
from tests.helpers import load_tokenizer_json

pytestmark = pytest.mark.gpu

PAD = 64                                                   # TKAMD_TEXT_PAD
N_STEPS = 48
NP = {"uint32": np.uint32, "int32": np.int32, "int64": np.int64}


def _on_emulation() -> bool:
    if os.environ.get("TKAMD_SIMT") != "1":
        return False
    import torch
    return not torch.cuda.is_available()


def _up(a: np.ndarray):
    """(what keeps the memory alive, device pointer) of a numpy array"""
    a = np.ascontiguousarray(a)
    if _on_emulation():
        return a, a.ctypes.data
    import torch
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    return t, t.data_ptr()


def _as_u32(i, dtype):
    """the id the device makes of a value: the bit pattern of an int32, 0xFFFFFFFF for an int64 that is no uint32"""
    if dtype == "int32":
        return int(i) & 0xFFFFFFFF
    return int(i) if 0 <= int(i) < 2 ** 32 else 0xFFFFFFFF


def _case_named(name, dec=dc.OWN):
    return dc.Case(next(i for i, (n, d) in enumerate(dc.DECODERS) if n == name and d == dec))


def _byte_level_case():
    return _case_named("gpt2_added_tokens")


_cache = {}


def _loaded(case):
    """(tokenizer on the device, decode of the oracle) of a case, once per process"""
    import tokenizers_amd as ta
    if case.k not in _cache:
        _cache[case.k] = (ta.Tokenizer.from_str(case.json, device=0), dsr.decoder_of(case.json))
    return _cache[case.k]


class Pair:
    """n device streams and their restatements, stepped together and compared at every step"""

    def __init__(self, case, n, skip, window=32, label=""):
        self.tk, self.decode = _loaded(case)
        self.n, self.skip, self.window, self.label = n, skip, window, label
        self.ds = self.tk.decode_stream(n, skip_special_tokens=skip, window=window)
        self.refs = [dsr.IntStream(self.decode, skip, window) for _ in range(n)]
        self.steps = 0
        self.seen = [0] * 5

    def step(self, ids, active=None, dtype="uint32"):
        keep = [_up(np.asarray(ids, dtype=NP[dtype]))]
        if active is not None:
            keep.append(_up(np.asarray(active, dtype=np.uint8)))
        text, d_status = self.ds.step_device(keep[0][1], keep[1][1] if active is not None else 0, dtype)
        assert d_status or self.n == 0
        return self.check(text, [_as_u32(i, dtype) for i in ids], active)

    def check(self, text, ids, active=None):
        raw, off, status = self.ds.read(text, slack=PAD)
        raw, off = raw.tobytes(), [int(x) for x in off]
        where = f"{self.label} skip={self.skip} step {self.steps}"
        assert text.n_docs == self.n and len(off) == self.n + 1, where
        assert off[0] == 0 and off[-1] == text.n_bytes == text.n_bytes_device(), (where, off[:3], off[-1], text.n_bytes)
        assert all(a <= b for a, b in zip(off[:-1], off[1:])), where
        assert raw[text.n_bytes:] == b"\0" * PAD, where
        got = [(int(status[i]), raw[off[i]:off[i + 1]]) for i in range(self.n)]
        exp = [self.refs[i].step(ids[i]) if active is None or active[i] else (dsr.INACTIVE, b"") for i in range(self.n)]
        bad = [(i, got[i], exp[i]) for i in range(self.n) if got[i] != exp[i]]
        assert not bad, f"{where}: {len(bad)} of {self.n} streams differ, first (stream, got, expected) {bad[0]!r}"
        for s, c in got:
            self.seen[s] += 1
            c.decode("utf-8")                                  # strict: a chunk is valid UTF-8
        self.steps += 1
        return got

    def check_state(self):
        for i, r in enumerate(self.refs):
            assert self.ds.peek(i) == r.state(), (self.label, i, self.ds.peek(i), r.state())

    def run(self, seqs, n_steps=N_STEPS, active=None):
        """stream i steps through seqs[i]"""
        for j in range(n_steps):
            self.step([q[j] for q in seqs], None if active is None else active(j))
        self.check_state()


def _spread(seqs, n, n_steps):
    """n sequences of n_steps ids out of a few: stream i takes seqs[i % m], started i // m ids later"""
    m = len(seqs)
    return [(seqs[i % m][(i // m) % 7:] + seqs[(i + 1) % m])[:n_steps] for i in range(n)]


@pytest.mark.parametrize("k", range(len(dc.DECODERS)), ids=dc.case_id)
def test_streams_vs_restatement(k):
    """Every decoder case: its sequences as parallel streams, both skip values, 48 steps.  (A window of 64: a stream that has met
    InvalidPrefix holds every id back from then on, as the reference's does.)"""
    case = dc.Case(k)
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(500 + k), N_STEPS)]
    seen = [0] * 5
    for skip in (True, False):
        p = Pair(case, len(seqs), skip, window=64, label=dc.case_id(k))
        p.run(seqs)
        seen = [a + b for a, b in zip(seen, p.seen)]
    assert seen[dsr.CHUNK] > 0 and seen[dsr.INACTIVE] == 0 and seen[dsr.WINDOW_FULL] == 0, seen


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_stream_counts_at_lane_wavefront_and_workgroup_edges(n):
    case = _byte_level_case()
    base = [q for _, q in dsr.sequences(case, dc.rng_for(901), N_STEPS)]
    n_steps = 48 if n <= 65 else 12
    p = Pair(case, n, True, label=f"{n} streams")
    p.run(_spread(base, n, n_steps), n_steps)
    if n:
        assert p.seen[dsr.CHUNK] and p.seen[dsr.NOTHING], p.seen
    else:
        assert p.steps == n_steps


def test_active_mask_that_changes_every_step():
    """streams that sit steps out -- one of them from the start, all of them on some steps -- keep their state and report 2"""
    case = _case_named("bpe_ws_byte_fallback", dc.DECODERS[7][1])
    base = [q for _, q in dsr.sequences(case, dc.rng_for(902), N_STEPS)]
    n = 70
    rng = dc.rng_for(903)
    masks = rng.integers(0, 2, size=(N_STEPS, n)).astype(np.uint8)
    masks[:, 5] = 0                                            # never stepped
    masks[:, 6] = 1
    masks[3] = masks[17] = masks[18] = 0                       # nobody steps
    masks[:4, 66] = 0
    p = Pair(case, n, False, label="mask")
    p.run(_spread(base, n, N_STEPS), N_STEPS, active=lambda j: masks[j])
    assert p.seen[dsr.INACTIVE] == int((masks == 0).sum()) and p.seen[dsr.CHUNK] and p.ds.peek(5) == ([], 0, 0)


def test_a_full_window_sticks_one_stream_until_it_alone_is_reset():
    case = _byte_level_case()
    sp, w = case.specials[0], case.words
    p = Pair(case, 3, True, window=4, label="window=4")
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


def test_window_of_two():
    case = _byte_level_case()
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(904), N_STEPS)]
    p = Pair(case, len(seqs), False, window=2, label="window=2")
    p.run(seqs)
    assert p.seen[dsr.CHUNK] and p.seen[dsr.WINDOW_FULL], p.seen      # (a character split over three tokens does not fit)


def test_invalid_prefix_on_one_stream_among_healthy_ones():
    """spm_bpe_llama2 ([Replace, ByteFallback, Fuse, Strip]): a sequence the restatement -- and the wheel -- answer with InvalidPrefix,
    between streams of plain words; the stream goes on as the reference's state says."""
    case = _case_named("spm_bpe_llama2")
    decode = dsr.decoder_of(case.json)
    bad = None
    for _, q in dsr.sequences(case, dc.rng_for(500 + case.k), N_STEPS):
        r = dsr.IntStream(decode, False)
        if dsr.INVALID_PREFIX in [r.step(i)[0] for i in q]:
            bad = q
            break
    assert bad is not None
    rng = dc.rng_for(905)
    plain = [[dc._pick(rng, case.words) for _ in range(N_STEPS)] for _ in range(4)]
    p = Pair(case, 5, False, label="invalid prefix")
    p.run(plain[:2] + [bad] + plain[2:])
    assert p.seen[dsr.INVALID_PREFIX] >= 1 and p.seen[dsr.CHUNK] >= 4 * N_STEPS - 8, p.seen


def test_seed_then_steps():
    case = _case_named("bpe_ws_byte_fallback", dc.DECODERS[7][1])
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(906), N_STEPS)]
    p = Pair(case, len(seqs), True, window=8, label="seed")
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
def test_id_types_and_values_that_are_no_id(dtype):
    case = _byte_level_case()
    seqs = [list(q) for _, q in dsr.sequences(case, dc.rng_for(907), N_STEPS)]
    for i, q in enumerate(seqs):
        for j in range(i % 5, N_STEPS, 5):
            q[j] = (-1, -100, case.n_ids + 7)[(i + j) % 3]
            if dtype == "int64" and (i + j) % 4 == 0:
                q[j] = (2 ** 32, 2 ** 40, -2 ** 63, 2 ** 63 - 1)[(i + j) % 4]
    p = Pair(case, len(seqs), True, label=dtype)
    for j in range(N_STEPS):                                   # (an int32's bit pattern is the id: -1 is 0xFFFFFFFF, -100 one no vocabulary has either)
        p.step([q[j] for q in seqs], dtype=dtype)
    assert p.seen[dsr.CHUNK] and p.seen[dsr.NOTHING]
    p.check_state()


def test_a_decode_batch_device_call_between_two_steps_disturbs_nothing():
    case = _byte_level_case()
    tk, decode = _loaded(case)
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(908), N_STEPS)]
    p = Pair(case, len(seqs), True, label="interleaved")
    o = DecodeOracle(case.json)
    flat = [i for q in seqs for i in q]
    keep = [_up(np.asarray(flat, dtype=np.uint32)), _up(np.arange(0, len(flat), N_STEPS, dtype=np.int64)),
            _up(np.arange(N_STEPS, len(flat) + 1, N_STEPS, dtype=np.int64))]
    whole = [o.decode(q, True) for q in seqs]
    for j in range(16):
        ids = [q[j] for q in seqs]
        kept = [_up(np.asarray(ids, dtype=np.uint32))]
        text, _ = p.ds.step_device(kept[0][1], 0, "uint32")
        other = tk.decode_batch_device(keep[0][1], len(flat), keep[1][1], keep[2][1], len(seqs), skip_special_tokens=True)
        assert other.to_strings() == whole
        p.check(text, ids)                                     # the step's text and status, read behind the other call
        assert other.to_strings() == whole                     # ... and the other call's text behind the step's read
    p.check_state()


def test_two_stream_objects_on_one_handle():
    case = _case_named("bert_wordpiece_4000_specials")
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(909), N_STEPS)]
    a, b = Pair(case, len(seqs), True, label="a"), Pair(case, len(seqs), False, label="b")
    for j in range(N_STEPS):
        a.step([q[j] for q in seqs])
        if j % 3:
            b.step([q[N_STEPS - 1 - j] for q in seqs])
    a.check_state()
    b.check_state()


def test_a_step_after_reset_of_all_equals_a_fresh_object():
    case = _byte_level_case()
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(910), N_STEPS)]
    p = Pair(case, len(seqs), True, window=4, label="used")
    for j in range(9):
        p.step([q[j] for q in seqs[::-1]])
    for j in range(5):
        p.step([case.specials[0]] * len(seqs))                 # (everybody stuck)
    assert p.seen[dsr.WINDOW_FULL]
    p.ds.reset()
    for r in p.refs:
        r.reset()
    fresh = Pair(case, len(seqs), True, window=4, label="fresh")
    for j in range(12):
        ids = [q[j] for q in seqs]
        assert p.step(ids) == fresh.step(ids)
    p.check_state()


def test_host_step_returns_strings_and_raises_with_what_the_healthy_streams_got():
    import tokenizers_amd as ta
    case = _byte_level_case()
    tk, decode = _loaded(case)
    sp, w = case.specials[0], case.words
    ds = tk.decode_stream(4, skip_special_tokens=True, window=2)
    refs = [dsr.IntStream(decode, True, 2) for _ in range(4)]

    def expect(ids, active=None):
        out = [refs[i].step(ids[i]) if active is None or active[i] else (2, b"") for i in range(4)]
        return [s for s, _ in out], [c.decode() if s == 1 else None for s, c in out]

    for ids, active in (([w[50], sp, w[51], w[52]], None), (np.array([w[53], sp, w[54], w[55]], dtype=np.int64), [1, 1, 0, 1])):
        status, chunks = expect(list(ids), active)
        assert max(status) < 3 and ds.step(ids, active) == chunks
    ids = [w[56], sp, w[57], w[58]]                            # the third special does not fit stream 1's window of two
    status, chunks = expect(ids)
    assert status[1] == 4
    with pytest.raises(ta.DecodeStreamError, match="stream 1: window full") as e:
        ds.step(ids)
    assert e.value.status == status and e.value.chunks == chunks and chunks[0] is not None
    ds.reset([1])
    refs[1].reset()
    assert ds.step(ids) == expect(ids)[1]
    with pytest.raises(ValueError, match="one id per stream"):
        ds.step([1, 2, 3])


@pytest.mark.needs_hw
def test_step_tensor():
    import torch
    case = _byte_level_case()
    tk, decode = _loaded(case)
    seqs = [q for _, q in dsr.sequences(case, dc.rng_for(911), N_STEPS)]
    n = len(seqs)
    ds = tk.decode_stream(n, skip_special_tokens=True)
    refs = [dsr.IntStream(decode, True) for _ in range(n)]
    for j in range(N_STEPS):
        ids = torch.tensor([q[j] for q in seqs], dtype=torch.int64 if j % 2 else torch.int32, device="cuda")
        active = None if j % 3 else torch.tensor([(i + j) % 4 != 0 for i in range(n)], device="cuda")
        text, status = ds.step_tensor(ids, active)
        exp = [refs[i].step(seqs[i][j]) if active is None or bool(active[i]) else (2, b"") for i in range(n)]
        assert status.cpu().tolist() == [s for s, _ in exp]
        assert text.to_strings() == [c.decode() for _, c in exp]
        assert text.bytes_tensor().cpu().numpy().tobytes() == b"".join(c for _, c in exp)
    with pytest.raises(TypeError):
        ds.step_tensor(torch.zeros(n, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        ds.step_tensor(torch.zeros(n + 1, dtype=torch.int64, device="cuda"))


def test_refusals():
    import tokenizers_amd as ta
    case = _byte_level_case()
    tk, _ = _loaded(case)
    with pytest.raises(ta.DeviceError, match="host-only tokenizer handle"):
        ta.Tokenizer.from_str(case.json, device=-1).decode_stream(4)
    meta = ta.Tokenizer.from_str(load_tokenizer_json("nfkc_spm_bpe"), device=0)
    with pytest.raises(ta.UnsupportedError, match="decode_batch: .*Metaspace") as e:
        meta.decode_stream(4)
    with pytest.raises(ta.UnsupportedError) as e2:
        meta.decode_batch([[1, 2]])
    assert str(e.value) == str(e2.value)                       # decode_batch's own message
    with pytest.raises(ValueError, match="at least 2 ids"):
        tk.decode_stream(4, window=1)
    ds = tk.decode_stream(4, window=3)
    with pytest.raises(ValueError, match="a seed of 4 ids does not fit the window of 3"):
        ds.seed(0, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="no stream 4"):
        ds.seed(4, [1])
    with pytest.raises(ValueError, match="no stream -1"):
        ds.reset([0, -1])
    with pytest.raises(ValueError, match="null ids"):
        ds.step_device(0)
    assert ds.step([case.words[3]] * 4) == [tk.decode([case.words[3]])] * 4      # (and the object is sound behind them)
