"""Inputs for the decode_batch tests (tests/test_decode_oracle_cases.py against the reference wheel on the CPU,
tests/test_decode_gpu.py against the oracle on the device): every decoder shape build_decode_tables folds into tables, over id
sequences whose hard places are indices -- k_decode_first / k_decode_byte_runs / k_decode_dups mark one bit per token in 32-token
mask words, k_decode_len and k_decode_copy work in 256-token blocks, k_scan_single takes 1024 block sums in one pass.
Plain module, fully seeded: the same (case, seed) gives the same sequences everywhere."""
import json

import numpy as np

from tests.helpers import N, load_tokenizer_json

OWN = "own"                    # the decoder section the fixture tokenizer carries (null included)


def _seq(*members):
    return {"type": "Sequence", "decoders": list(members)}


def _replace(a, b):
    return {"type": "Replace", "pattern": {"String": a}, "content": b}


def _strip(c, start, stop):
    return {"type": "Strip", "content": c, "start": start, "stop": stop}


def _ctc(pad, delim, cleanup):
    return {"type": "CTC", "pad_token": pad, "word_delimiter_token": delim, "cleanup": cleanup}


_BF, _FUSE = {"type": "ByteFallback"}, {"type": "Fuse"}

# (fixture tokenizer, decoder section).  CTC on wordlevel_whitespace_c1: "hai" and "'" are ids 5 and 6 (whole tokens, what
# oracle/make_decode_golden.py picks); "s" and "e" are one-char strings that also occur inside other tokens.
DECODERS = [
    # the decoder overrides of oracle/make_decode_golden.py
    ("bert_wordpiece_4000_specials", {"type": "WordPiece", "prefix": "##", "cleanup": True}),
    ("bert_wordpiece_4000_specials", {"type": "WordPiece", "prefix": "##", "cleanup": False}),
    ("bpe_wssplit_suffix_fuse", {"type": "BPEDecoder", "suffix": "</w>"}),
    ("bpe_bert_affixes", {"type": "BPEDecoder", "suffix": "</w>"}),
    ("bpe_ws_byte_fallback", _BF),
    ("bpe_ws_byte_fallback", _seq(_BF, _FUSE)),
    ("bpe_ws_unk", _FUSE),
    ("bpe_ws_byte_fallback", _seq(_replace("a", " "), _BF, _FUSE, _strip(" ", 1, 0))),
    ("bpe_ws_byte_fallback", _seq(_BF, _FUSE, _strip("t", 1, 0))),
    ("bpe_ws_unk", _strip("t", 2, 0)),
    ("bpe_ws_unk", _strip("s", 0, 1)),
    ("bpe_ws_unk", _replace("th", "TH-")),
    ("bpe_ws_unk", _seq(_replace("e", "3"), _strip("3", 1, 0))),
    ("wordlevel_whitespace_c1", _ctc("hai", "'", True)),
    ("wordlevel_whitespace_c1", _ctc("hai", "'", False)),
    # a one-letter suffix that occurs inside tokens
    ("bpe_wssplit_suffix_fuse", {"type": "BPEDecoder", "suffix": "e"}),
    ("bert_wordpiece_4000_specials", {"type": "WordPiece", "prefix": "", "cleanup": True}),
    ("bert_wordpiece_4000_specials", {"type": "WordPiece", "prefix": "#", "cleanup": True}),
    # CTC: pad / delimiter inside other tokens, an empty pad, an empty delimiter
    ("wordlevel_whitespace_c1", _ctc("s", "e", True)),
    ("wordlevel_whitespace_c1", _ctc("s", "e", False)),
    ("wordlevel_whitespace_c1", _ctc("", "'", True)),
    ("wordlevel_whitespace_c1", _ctc("hai", "", True)),
    ("wordlevel_whitespace_c1", _ctc("hai", "", False)),
    # the SentencePiece chain: the stripped char has a byte token of its own (<0x20>, <0x74>, <0x61>) AND comes out of the Replace
    ("bpe_ws_byte_fallback", _seq(_replace("e", " "), _BF, _FUSE, _strip(" ", 1, 0))),
    ("bpe_ws_byte_fallback", _seq(_replace("a", "t"), _BF, _FUSE, _strip("t", 1, 0))),
    ("bpe_ws_byte_fallback", _seq(_replace("e", "a"), _BF, _FUSE, _strip("a", 1, 0))),
    # a per-token Strip in front of ByteFallback: "<" off "<0xXX>" leaves no byte token behind (no token is "<" alone: Strip(c, 1, 1)
    # of the one-char token c panics in the reference)
    ("bpe_ws_byte_fallback", _seq(_strip("<", 1, 1), _BF, _FUSE)),
    # a trailing per-token Strip that leaves the token "s" empty: an empty token still ends a byte run
    ("bpe_ws_byte_fallback", _seq(_strip("s", 0, 1), _BF, _FUSE)),
    ("spm_bpe_llama2", OWN),
    ("gpt2_added_tokens", OWN),
    ("llama3_small_6000_specials", OWN),
    ("bert_wordpiece_4000_specials", OWN),
]

# one large batch per decoder family: index into DECODERS
LARGE = {7: "ByteFallback chain", 13: "CTC", 2: "BPEDecoder", 0: "WordPiece"}


def case_id(k):
    name, dec = DECODERS[k]
    if dec == OWN:
        return f"{k}-{name}-own"
    tag = dec["type"]
    if tag == "Sequence":
        tag = "+".join(m["type"] for m in dec["decoders"])
    return f"{k}-{name}-{tag}"


# bytes for runs of <0xXX> tokens: characters of one to four bytes, truncated ones, overlong forms, a surrogate, a value above
# U+10FFFF, lone continuation bytes, bytes that never occur in UTF-8
_BYTE_PIECES = ["a".encode(), " ".encode(), "t".encode(), "é".encode(), "中文".encode(), "€".encode(), "\U0001f600".encode(),
                b"\xe4\xb8", b"\xf0\x9f\x98", b"\xc3", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"\xbf\x80",
                b"\xff", b"\xf5"]
_VALID_PIECES = _BYTE_PIECES[:7]


class Case:
    """One (tokenizer, decoder) pair: its tokenizer.json text and what sequences() needs to know about its vocabulary."""

    def __init__(self, k):
        self.k = k
        self.name, dec = DECODERS[k]
        d = json.loads(load_tokenizer_json(self.name))
        if dec != OWN:
            d["decoder"] = dec
        self.decoder = d.get("decoder")
        self.json = json.dumps(d)
        id2tok = {i: t for t, i in d["model"]["vocab"].items()}
        special = set()
        for a in d.get("added_tokens") or []:
            id2tok[a["id"]] = a["content"]
            if a.get("special"):
                special.add(a["content"])
        self.id2tok = id2tok
        self.n_ids = max(id2tok) + 1
        self.specials = sorted(i for i, t in id2tok.items() if t in special)
        self.absent = [self.n_ids + 1, self.n_ids + 3] + [i for i in range(self.n_ids) if i not in id2tok][:2]
        self.byte_id = {}
        for i, t in id2tok.items():
            if len(t) == 6 and t.startswith("<0x") and t.endswith(">"):
                try:
                    self.byte_id[int(t[3:5], 16)] = i
                except ValueError:
                    pass
        not_word = set(self.specials) | set(self.byte_id.values())
        self.words = [i for i in sorted(id2tok) if i not in not_word]
        members = self.decoder["decoders"] if self.decoder and self.decoder["type"] == "Sequence" else [self.decoder] if self.decoder else []
        self.members = members
        kinds = [m["type"] for m in members]
        self.has_bytes = "ByteFallback" in kinds and len(self.byte_id) == 256
        self.dedup = kinds == ["CTC"]
        self.from_end = kinds == ["BPEDecoder"]
        self.large = k in LARGE
        # a Strip with start >= 1: the ids whose token begins with the stripped char, by itself or through a Replace in front of it
        self.strip_char, self.strip_heads = None, []
        strips = [m for m in members if m["type"] == "Strip" and m["start"] >= 1]
        if strips:
            c = strips[-1]["content"]
            self.strip_char = c
            pre = [c] + [m["pattern"]["String"] for m in members if m["type"] == "Replace" and m["content"] == c]
            exact = [i for i in self.words if id2tok[i] in pre]
            begins = [i for i in self.words if id2tok[i] not in pre and any(id2tok[i].startswith(p) for p in pre)]
            twice = [i for i in self.words if any(id2tok[i].startswith(p + q) for p in pre for q in pre)]
            self.strip_heads = exact[:2] + begins[:2] + twice[:1]
        # CTC: a few ids to draw chains from -- the first dozen, and whatever holds the pad or the delimiter
        self.ctc_ids = list(range(12))
        if self.dedup:
            for s in (self.decoder["pad_token"], self.decoder["word_delimiter_token"]):
                self.ctc_ids += [i for i in self.words if s and s in id2tok[i]][:3]


class Batch:
    """One decode_batch call: `seqs`, and `featured` -- the documents built around an edge (every aligned and every leading-Strip
    one), which the batch-independence test decodes on their own."""

    def __init__(self, name, seqs, featured=()):
        self.name, self.seqs, self.featured = name, seqs, list(featured)

    @property
    def n_tokens(self):
        return sum(len(q) for q in self.seqs)


def _pick(rng, xs):
    return int(xs[int(rng.integers(0, len(xs)))])


def _dropped(case, rng):
    """an id the decoder never sees: no such token, or a special (dropped under skip_special_tokens only)"""
    if case.specials and rng.random() < 0.5:
        return _pick(rng, case.specials)
    return _pick(rng, case.absent)


def _byte_run(case, rng, n, valid=None):
    """ids of n <0xXX> tokens: pieces of _BYTE_PIECES end to end, cut at n bytes (so the last character may be truncated)"""
    raw = bytearray()
    pieces = _VALID_PIECES if valid else _BYTE_PIECES
    while len(raw) < n:
        p = pieces[int(rng.integers(0, len(pieces)))]
        if valid and len(raw) + len(p) > n:
            p = b"a"
        raw += p
    return [case.byte_id[b] for b in raw[:n]]


def _run(case, rng, n):
    """n tokens of the kind that makes this decoder look past one token: a byte run, a chain of equal ids, or plain words"""
    if case.has_bytes:
        return _byte_run(case, rng, n, valid=rng.random() < 0.4)
    if case.dedup:
        return [_pick(rng, case.ctc_ids)] * n
    return [_pick(rng, case.words) for _ in range(n)]


def _random_seq(case, rng, n):
    return [int(x) for x in rng.integers(0, case.n_ids + 4, size=n)]


def _mixed_seq(case, rng, n):
    """n ids of everything this decoder branches on: runs, words, dropped ids, uniform ids"""
    q = []
    while len(q) < n:
        r = rng.random()
        if r < 0.45:
            q += _run(case, rng, int(rng.integers(1, 9)))
        elif r < 0.75:
            q.append(_pick(rng, case.words))
        elif r < 0.9:
            q.append(_dropped(case, rng))
        else:
            q += _random_seq(case, rng, int(rng.integers(1, 4)))
    return q[:n]


def _filled(case, rng, n_tok, max_len=400):
    """sequences of 1..max_len ids with exactly n_tok ids in all"""
    seqs, left = [], n_tok
    while left > 0:
        n = min(left, int(rng.integers(1, max_len + 1)))
        seqs.append(_mixed_seq(case, rng, n))
        left -= n
    return seqs


def _padding_docs(case, rng, n_tok):
    """documents of 0..12 ordinary tokens, n_tok in all: what stands in front of an aligned document"""
    seqs, left = [], n_tok
    while left > 0:
        n = min(left, int(rng.integers(0, 13)))
        seqs.append([_pick(rng, case.words) for _ in range(n)])
        left -= n
    return seqs


def _aligned(case, rng, mode, delta):
    """One batch with a run at every edge 32k + delta (k = 1..9) and 256k + delta (k = 1, 2) of the FLAT token index: it starts at the
    edge, ends at it, or straddles it.  The run is what this decoder marks: <0xXX> tokens (badmask), equal ids with dropped ids among
    them (dupmask), and in every case the first and the last kept token of its document (firstmask), with dropped ids outside them."""
    edges = sorted({32 * k + delta for k in range(1, 10)} | {256 * k + delta for k in (1, 2)})
    seqs, featured, pos = [], [], 0
    for g in edges:
        n = int(rng.integers(2, 9))
        run = _run(case, rng, n)
        if case.dedup and rng.random() < 0.5:                   # dropped ids inside a chain do not end it
            run = run[:1] + [_dropped(case, rng)] + run[1:-1]
            n = len(run)
        start = {"start": g, "end": g - n + 1, "straddle": g - n // 2}[mode]
        lead = [_dropped(case, rng) for _ in range(int(rng.integers(0, 3)))]
        tail = [_dropped(case, rng) for _ in range(int(rng.integers(0, 3)))]
        doc_start = start - len(lead)
        assert doc_start >= pos, (g, mode, delta, pos)
        seqs += _padding_docs(case, rng, doc_start - pos)
        featured.append(len(seqs))
        seqs.append(lead + run + tail)
        pos = doc_start + len(lead) + n + len(tail)
        flat = [i for q in seqs for i in q]
        assert flat[start:start + n] == run
    return Batch(f"aligned-{mode}{delta:+d}", seqs, featured)


def _byte_run_seqs(case, rng):
    seqs = []
    for j in range(36):
        n_runs = int(rng.integers(1, 4))
        q = []
        for r in range(n_runs):
            n = int(rng.integers(1, 81)) if j % 2 else int(rng.integers(1, 9))
            if r or j % 3 == 0:                                 # (else the run is the very start of the sequence)
                sep = int(rng.integers(0, 4))
                if sep == 0:
                    q.append(_pick(rng, case.words))
                elif sep == 1:
                    q += [_dropped(case, rng) for _ in range(int(rng.integers(1, 3)))]      # does not end a run in the reference
                elif sep == 2:
                    q += [_pick(rng, case.words), _dropped(case, rng)]
            q += _byte_run(case, rng, n, valid=rng.random() < 0.35)
        if j % 4 == 1:                                          # (else the run is the very end of the sequence)
            q.append(_pick(rng, case.words))
        elif j % 4 == 2:
            q.append(_dropped(case, rng))
        seqs.append(q)
    return seqs


def _ctc_seqs(case, rng):
    seqs = []
    for _ in range(30):
        q, cur = [], _pick(rng, case.ctc_ids)
        for _ in range(int(rng.integers(1, 120))):
            if rng.random() < 0.4:
                cur = _pick(rng, case.ctc_ids)
            q.append(cur)
            if rng.random() < 0.15:
                q.append(_dropped(case, rng))
        seqs.append(q)
    return seqs


def _leading_strip_seqs(case, rng):
    """The stripped char as the first kept token -- a byte token, a token that is the char, one that begins with it; once and twice; in
    front of a byte run that is UTF-8 and one that is not; at the very start, behind an id without a token, behind a special."""
    heads = [[i] for i in case.strip_heads]
    if case.has_bytes and len(case.strip_char.encode()) == 1:
        cb = case.byte_id[case.strip_char.encode()[0]]
        heads += [[cb], [cb, cb]] + [[cb, h[0]] for h in heads[:2]] + [[h[0], cb] for h in heads[:2]]
    heads += [[h[0], h[0]] for h in heads[:len(case.strip_heads)]]
    w = _pick(rng, case.words)
    tails = [[], [w]]
    if case.has_bytes:
        b = case.byte_id
        tails += [[b[0xC3], b[0xA9]], [b[0xC3]], [b[0xE4], b[0xB8]], [b[0xC3], b[0xA9], w], [b[0xC3], heads[-1][0]]]
    fronts = [[], [case.absent[0]]] + ([[case.specials[0]], [case.absent[0], case.specials[0]]] if case.specials else [])
    return [f + h + t for f in fronts for h in heads for t in tails]


def sequences(case, rng):
    """The small batches of one case: a list of Batch.  A few thousand tokens but for the three batches whose point is their size."""
    out = [Batch("uniform", [_random_seq(case, rng, int(n)) for n in [0, 1, 300] + list(rng.integers(0, 301, size=9))])]
    if case.byte_id:
        out.append(Batch("byte-runs", _byte_run_seqs(case, rng)))
    if case.dedup:
        out.append(Batch("ctc-chains", _ctc_seqs(case, rng)))
    for mode in ("start", "end", "straddle"):
        for delta in (-1, 0, 1):
            out.append(_aligned(case, rng, mode, delta))
    # document edges
    w = lambda n: [_pick(rng, case.words) for _ in range(n)]
    only_dropped = [[_dropped(case, rng) for _ in range(n)] for n in (1, 2, 33)]
    out.append(Batch("empties", [[], [], w(3), [], [], [], [], w(1), only_dropped[0], [], _mixed_seq(case, rng, 40), only_dropped[1], only_dropped[2], w(2), []]))
    out.append(Batch("all-empty", [[], [], []]))
    out.append(Batch("only-dropped", only_dropped))
    packed = [[_pick(rng, case.words)] if j % 7 else _run(case, rng, 1) for j in range(40)]
    out.append(Batch("one-token-x40", [w(5)] + packed + [[_dropped(case, rng)], []] + packed[:33] + [w(2)]))
    out.append(Batch("no-documents", []))
    out.append(Batch("tokens-256", _filled(case, rng, 256, max_len=60)))
    full = _filled(case, rng, 8192)
    out.append(Batch("tokens-8192", full))
    out.append(Batch("tokens-8193", full + [_run(case, rng, 1)]))
    if case.strip_char is not None:
        q = _leading_strip_seqs(case, rng)
        out.append(Batch("leading-strip", q, range(len(q))))
    for b in out:
        assert all(0 <= i < 2 ** 32 for q in b.seqs for i in q)
    assert [b.n_tokens for b in out if b.name.startswith("tokens-")] == [256, 8192, 8193]
    return out


def large_batch(case, rng, n_tok=None):
    """N(280_000) ids in sequences of 1..400: more than 1024 blocks of 256 tokens, so k_scan_single's block-sum scan takes a second pass
    (tests.helpers.N shrinks it under the emulation)."""
    return Batch("large", _filled(case, rng, N(280_000) if n_tok is None else n_tok))


def rng_for(k):
    return np.random.default_rng(7000 + k)
