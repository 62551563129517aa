"""The reference's streaming decode (tokenizers/src/tokenizer/mod.rs ``step_decode_stream``; Python ``tokenizers.decoders.DecodeStream``)
restated over oracle.decode_oracle.DecodeOracle, twice: with the text state the reference keeps (``TextStream``: ids, prefix,
prefix_index) and with the integer state the device keeps (``IntStream``: win, pe, pi -- the prefix is always the decode of the first
``pe`` ids of the window, so no text is stored).  tests/test_decode_stream_ref.py holds both to the wheel on the CPU;
tests/test_decode_stream_gpu.py holds the device to ``IntStream``.  Also the id sequences both tests step through.
Plain module, fully seeded."""
import numpy as np

from oracle.decode_oracle import DecodeOracle

FFFD = "�".encode("utf-8")

# what a step reports, as tkamd_decode_stream_step does
NOTHING, CHUNK, INACTIVE, INVALID_PREFIX, WINDOW_FULL = 0, 1, 2, 3, 4


class InvalidPrefix(Exception):
    """DecodeStreamError::InvalidPrefix"""


def decoder_of(json_str):
    """decode(ids, skip_special_tokens) -> the bytes of Tokenizer::decode's string (from_utf8_lossy applied: only the ByteLevel decoder
    can emit anything it changes)"""
    o = DecodeOracle(json_str)
    return lambda ids, skip: o.decode_bytes(ids, skip).decode("utf-8", "replace").encode("utf-8")


class TextStream:
    """step_decode_stream line by line: the state is the reference's (ids, prefix, prefix_index); ``ids`` = the constructor's ``ids=``"""

    def __init__(self, decode, skip, ids=()):
        self.decode, self.skip = decode, skip
        self.ids, self.prefix, self.prefix_index = [int(i) for i in ids], b"", 0

    def step(self, tid):
        if not self.prefix and self.ids:
            p = self.decode(self.ids, self.skip)
            if not p.endswith(FFFD):
                self.prefix, self.prefix_index = p, len(self.ids)
        self.ids.append(int(tid))
        s = self.decode(self.ids, self.skip)
        if len(s) > len(self.prefix) and not s.endswith(FFFD):
            if not s.startswith(self.prefix):
                raise InvalidPrefix()
            chunk = s[len(self.prefix):]
            new_index = len(self.ids) - self.prefix_index
            self.ids = self.ids[self.prefix_index:]
            self.prefix = self.decode(self.ids, self.skip)
            self.prefix_index = new_index
            return chunk
        return None


class IntStream:
    """The same step over (win, pe, pi): prefix == decode(win[:pe]) at every point, so a step decodes [0, pe), [0, n0) and [0, n) of the
    window and compares.  (pe and pi move together -- both become the ids in front of the step, or the window's length behind a drain;
    they are kept apart as the reference keeps a text and an index.)  ``window``: the ids the window may hold; a step that finds it full
    sticks the stream (status 4) until it is reset.  step() -> (status, chunk bytes)."""

    def __init__(self, decode, skip, window=32, ids=()):
        self.decode, self.skip, self.window = decode, skip, window
        self.seed(ids)

    def seed(self, ids=()):
        self.win, self.pe, self.pi, self.stuck = [int(i) for i in ids], 0, 0, False
        assert len(self.win) <= self.window

    reset = seed

    def step(self, tid):
        if self.stuck or len(self.win) >= self.window:
            self.stuck = True
            return WINDOW_FULL, b""
        n0 = len(self.win)
        pre = self.decode(self.win[:self.pe], self.skip)
        if not pre and n0:
            p = self.decode(self.win, self.skip)
            if not p.endswith(FFFD):
                pre, self.pe, self.pi = p, n0, n0
        self.win.append(int(tid))
        s = self.decode(self.win, self.skip)
        if len(s) > len(pre) and not s.endswith(FFFD):
            if not s.startswith(pre):
                return INVALID_PREFIX, b""
            self.win = self.win[self.pi:]
            self.pe = self.pi = len(self.win)
            return CHUNK, s[len(pre):]
        return NOTHING, b""

    def state(self):
        return list(self.win), self.pe, self.pi


# ---- the id sequences of one decoder case (tests/decode_cases.py Case) ------------------------------------------------------------

TEXT = "héllo wörld €uro 中文 naïve \U0001f600 the end, isn't it? \U0001f9d1‍\U0001f680 ok"


def _encode(case, n):
    """ids of TEXT by the case's own tokenizer where the wheel can encode with it, else None"""
    try:
        import tokenizers
        return [int(i) for i in tokenizers.Tokenizer.from_str(case.json).encode(TEXT, add_special_tokens=False).ids][:n]
    except Exception:
        return None


def _bytes_as_ids(case, raw):
    return [case.byte_id[b] for b in raw]


def sequences(case, rng, n_steps=48):
    """[(name, ids)]: every sequence has n_steps ids, all of them uint32.  What they hold: text with 2-, 3- and 4-byte characters (as the
    tokenizer encodes it, or -- where it cannot or the wheel is absent -- as <0xXX> runs or words), random ids, byte runs that are
    complete, cut short and invalid, runs of special tokens, equal ids in a row (CTC's dedup across a drain of the window)."""
    from tests import decode_cases as dc
    out = []

    def add(name, q):
        q = [int(i) for i in q]
        while len(q) < n_steps:
            q.append(dc._pick(rng, case.words))
        out.append((name, q[:n_steps]))

    enc = _encode(case, n_steps)
    if enc:
        add("text", enc)
    add("words", [dc._pick(rng, case.words) for _ in range(n_steps)])
    add("random", dc._random_seq(case, rng, n_steps))
    add("mixed", dc._mixed_seq(case, rng, n_steps))
    if case.byte_id and len(case.byte_id) == 256:
        w = lambda: dc._pick(rng, case.words)
        raw = TEXT.encode("utf-8")
        add("bytes-text", _bytes_as_ids(case, raw))
        add("bytes-complete", [w()] + _bytes_as_ids(case, "é€\U0001f600".encode()) + [w(), w()] + _bytes_as_ids(case, "中".encode()) + [w()])
        add("bytes-cut-short", [w()] + _bytes_as_ids(case, b"\xe2\x82") + [w(), w()] + _bytes_as_ids(case, b"\xf0\x9f\x98") + [w()] + _bytes_as_ids(case, b"\xc3") + [w()])
        add("bytes-invalid", [w()] + _bytes_as_ids(case, b"\xff\x80") + [w()] + _bytes_as_ids(case, b"\xc0\x80\xed\xa0\x80") + [w()] + _bytes_as_ids(case, b"a\xf5") + [w()])
        add("bytes-first", _bytes_as_ids(case, b"\xe4\xb8\xad\xe6\x96") + [w()] + _bytes_as_ids(case, b"\x87"))
        add("bytes-random", dc._byte_run(case, rng, n_steps))
    if case.specials:
        sp = case.specials
        add("specials", [sp[0]] * 5 + [dc._pick(rng, case.words)] + [sp[-1], sp[0], sp[-1]] + [dc._pick(rng, case.words)] * 2 + [sp[0]] * 7)
        add("specials-first", [sp[-1]] * 3 + [dc._pick(rng, case.words) for _ in range(4)] + [sp[0]])
    if case.dedup:
        a, b = dc._pick(rng, case.ctc_ids), dc._pick(rng, case.ctc_ids)
        add("repeats", [a] * 6 + [b] * 2 + [a, a, b, b, b, a] + [dc._dropped(case, rng), a, a] + [b] * 9)
    if case.strip_heads:
        h = case.strip_heads
        add("strip-heads", [h[0], h[0], h[-1]] + [dc._pick(rng, case.words), h[0], h[-1], h[0]] * 3)
    add("absent", [case.absent[0], case.absent[1]] + [dc._pick(rng, case.words), case.absent[0]] * 4)
    return out
