"""Inputs for the tests of the word-aligned GPT-2 pre-tokenizer (tests/test_pretok_gpt2_words.py on the CPU,
tests/test_gpu_pretok_gpt2_words.py on the device): one lane of k_pretok_gpt2_seq owns 64 bytes of text, a wavefront 4,096,
a workgroup 16,384, and what is hard sits where those meet."""
import numpy as np

LANE, WAVE, GROUP = 64, 4096, 16384

# ASCII letters, digits, the six whitespace bytes, the apostrophe with each contraction suffix, and 2-, 3- and 4-byte code points
# of the classes letter / number / whitespace / other (no whitespace character has four bytes)
ALPHA = (list("abzAZstdmlvre") + list("0189") + [" ", " ", " ", "\t", "\n", "\v", "\f", "\r"] +
         ["'", "'s", "'t", "'m", "'d", "'re", "'ve", "'ll", "'S", "'x"] + list("!-_.,?") +
         ["\u00e9", "\u0416", "\u00b2", "\u0663", "\u00a0", "\u0085", "\u00a7", "\u00d7",                  # 2 bytes: L L N N S S other other
          "\u4e2d", "\u0905", "\u2167", "\u0969", "\u3000", "\u2003", "\u2028", "\u20ac", "\u2014",       # 3 bytes: L L N N S S S other other
          "\U0001d400", "\U00010400", "\U0001d7ce", "\U00010107", "\U0001f601", "\U0001f680"])            # 4 bytes: L L N N other other


def random_docs(n, seed, max_len=24):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, size=n)
    picks = rng.integers(0, len(ALPHA), size=int(lens.sum()))
    out, k = [], 0
    for ln in lens.tolist():
        out.append("".join(ALPHA[i] for i in picks[k:k + ln].tolist()))
        k += ln
    return out


_FILL = ("the quick brown fox's 42 dogs   jump\tover\n lazy 7 cats, don't they? we've seen  it\r\n" * 3).encode()

# (bytes placed at the edge, whether a document starts with them)
FEATURES = [(s.encode("utf-8"), False) for s in
            ["\u00e9", "\u4e2d", "\U0001d400", "\u3000x", "\u0663", "\U0001f601", " \u4e2d\u4e2d", "    \u3000",     # a multi-byte code point
             "it's", "we're", "I'll", "'t", "x've ", "a'd'm",                                                      # a contraction
             "   a", " a", "\n  \n x", "     "]] + \
           [(s.encode("utf-8"), True) for s in ["x", " x", "'s", "\u4e2d", "  "]]                                  # a document start


def _filler(n, phase):
    reps = (n + phase) // len(_FILL) + 2
    return (_FILL * reps)[phase:phase + n]


def straddling_text(edges):
    """One text with one constructed case at every edge of `edges` (ascending byte positions, far enough apart): FEATURES x the offsets
    -8..+8, in that order, as many as there are edges.  A document boundary lies half way between two edges, so every case is a document
    (two where the feature starts one).  Returns (bytes, list of document offsets)."""
    cases = [(f, d, delta) for f, d in FEATURES for delta in range(-8, 9)]
    assert len(edges) >= len(cases), (len(edges), len(cases))
    out, off = bytearray(), [0]
    for j, (feat, doc, delta) in enumerate(cases):
        e = edges[j]
        end = (e + edges[j + 1]) // 2 if j + 1 < len(edges) else e + 64
        assert len(out) <= e + delta and e + delta + len(feat) <= end
        out += _filler(e + delta - len(out), j % 37)
        if doc:
            off.append(len(out))
        out += feat
        out += _filler(end - len(out), (5 * j) % 41)
        off.append(len(out))
    return bytes(out), off


N_CASES = len(FEATURES) * 17


def edges_of(kind, first=1):
    """N_CASES edges of one kind: lane edges that are no wavefront edge, wavefront edges that are no workgroup edge, workgroup edges."""
    step, coarser = {"lane": (LANE, WAVE), "wave": (WAVE, GROUP), "group": (GROUP, None)}[kind]
    out, k = [], first
    while len(out) < N_CASES:
        # lane edges 256 bytes apart: a case is up to 8 + 8 bytes on either side of its edge
        e = k * step * (4 if kind == "lane" else 1)
        if coarser is None or e % coarser:
            out.append(e)
        k += 1
    return out


def docs_of(text, off):
    return [text[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
