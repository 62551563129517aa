"""The restatement of the reference's streaming decode (tests/decode_stream_ref.py: the text-state form and the integer-state form the
device runs) against the reference wheel's ``tokenizers.decoders.DecodeStream``, token by token, on the sequences the device test
steps through: every decoder case of tests/decode_cases.py, both skip_special_tokens values.  A step on which the wheel raises
InvalidPrefix counts as compared: the restatement must report it on that very step, and both go on from the state the reference leaves.
``seed`` is compared with the wheel too: the constructor of the wheel this was written against (0.22.2) takes ``ids=``; an older one that
does not is compared with the text-state restatement alone.
This is what lets tests/test_decode_stream_gpu.py compare the device with the restatement alone."""
import pytest

from tests import decode_cases as dc
from tests import decode_stream_ref as dsr

N_STEPS = 48
WINDOW = 64                                                 # (no sequence here fills it: the wheel's window has no limit)

_KEYS = ("none", "chunk", "invalid", "window")
_done = {}                                                  # case -> what its inputs produced on the WHEEL's side (None: the wheel cannot build it)
_seen = dict.fromkeys(_KEYS, 0)                             # ... of the case being run


def _wheel_stream(ref_tokenizers, skip, ids=None):
    DS = ref_tokenizers.decoders.DecodeStream
    if ids is None:
        return DS(skip_special_tokens=skip)
    try:
        return DS(ids=list(ids), skip_special_tokens=skip)
    except TypeError:
        return None


def _run(ref_tokenizers, ref, decode, skip, name, q, seed=None):
    """One sequence through the wheel, the text form and the integer form at once; the wheel's window is not visible, so the longest
    window is the text form's, which is held to the wheel's chunks at every step."""
    wheel = _wheel_stream(ref_tokenizers, skip, seed)
    text = dsr.TextStream(decode, skip, seed or ())
    ints = dsr.IntStream(decode, skip, WINDOW, seed or ())
    for j, tid in enumerate(q):
        where = f"{name} skip={skip} step {j} id {tid}"
        try:
            exp = text.step(tid)
            exp_status = dsr.CHUNK if exp is not None else dsr.NOTHING
        except dsr.InvalidPrefix:
            exp, exp_status = None, dsr.INVALID_PREFIX
        if wheel is not None:
            try:
                got = wheel.step(ref, tid)
                got_status = dsr.CHUNK if got is not None else dsr.NOTHING
                got = got.encode("utf-8") if got is not None else None
            except Exception as e:
                assert "Invalid prefix" in str(e), (where, e)
                got, got_status = None, dsr.INVALID_PREFIX
            assert (got_status, got) == (exp_status, exp), (where, got_status, got, exp_status, exp)
            _seen[{dsr.NOTHING: "none", dsr.CHUNK: "chunk", dsr.INVALID_PREFIX: "invalid"}[got_status]] += 1
            _seen["window"] = max(_seen["window"], len(text.ids))
        status, chunk = ints.step(tid)
        assert (status, chunk) == (exp_status, exp or b""), (where, status, chunk, exp_status, exp)
        assert ints.win == text.ids and ints.pe == ints.pi == text.prefix_index, (where, ints.state(), text.ids, text.prefix_index)
        assert decode(ints.win[:ints.pe], skip) == text.prefix, where
    return wheel is not None


def _case(k, ref_tokenizers):
    """every sequence of case k through the three; once per process"""
    if k in _done:
        return _done[k]
    case = dc.Case(k)
    try:
        ref = ref_tokenizers.Tokenizer.from_str(case.json)
    except Exception:                                           # (a decoder section this wheel cannot build: nothing to hold it to)
        _done[k] = None
        return None
    _seen.update(dict.fromkeys(_KEYS, 0))
    decode = dsr.decoder_of(case.json)
    seqs = dsr.sequences(case, dc.rng_for(500 + k), N_STEPS)
    assert len(seqs) >= 4
    for name, q in seqs:
        for skip in (True, False):
            _run(ref_tokenizers, ref, decode, skip, name, q)
    # seed: the constructor's ids=, then steps
    for name, q in seqs[:3]:
        for n_seed in (1, 3):
            _run(ref_tokenizers, ref, decode, True, f"{name} seeded with {n_seed}", q[n_seed:], seed=q[:n_seed])
    _done[k] = dict(_seen)
    return _done[k]


@pytest.mark.parametrize("k", range(len(dc.DECODERS)), ids=dc.case_id)
def test_restatement_matches_the_wheels_decode_stream(k, ref_tokenizers):
    if _case(k, ref_tokenizers) is None:
        pytest.skip("the wheel does not build this decoder section")


def test_the_inputs_reach_every_outcome_on_the_wheel(ref_tokenizers):
    """Over the whole file the wheel itself returned None, returned a chunk, raised InvalidPrefix and held back four ids or more: none
    of the comparisons is vacuous.  (The cases run above are not run again in the same process.)"""
    got = [r for r in (_case(k, ref_tokenizers) for k in range(len(dc.DECODERS))) if r is not None]
    assert len(got) >= len(dc.DECODERS) - 2
    tot = {key: (max if key == "window" else sum)(r[key] for r in got) for key in _KEYS}
    assert tot["none"] >= 1 and tot["chunk"] >= 1 and tot["invalid"] >= 1 and tot["window"] >= 4, tot
    print(tot)


def test_the_window_limit_of_the_integer_form():
    """what the reference has no word for: a window that is full sticks the stream until it is reset"""
    k = next(i for i, (name, dec) in enumerate(dc.DECODERS) if name == "gpt2_added_tokens" and dec == dc.OWN)
    case = dc.Case(k)
    assert case.specials
    s = dsr.IntStream(dsr.decoder_of(case.json), True, window=4)
    sp, w = case.specials[0], case.words[40]
    assert [s.step(sp)[0] for _ in range(5)] == [0, 0, 0, 0, 4] and s.state() == ([sp] * 4, 3, 3)
    assert s.step(w) == (4, b"")
    s.reset()
    assert s.step(w)[0] == 1 and s.state() == ([w], 1, 1)


def test_the_sequences_are_seeded():
    a = dsr.sequences(dc.Case(7), dc.rng_for(507), N_STEPS)
    assert a == dsr.sequences(dc.Case(7), dc.rng_for(507), N_STEPS) and all(len(q) == N_STEPS for _, q in a)
