"""Inputs shared by tests/test_nfc.py (the core against the wheel, CPU) and tests/test_nfc_gpu.py (the kernels against the wheel): the
ACTIVE set of tokenizers_amd/csrc/nfc_tables.inc -- chars whose canonical combining class is not 0 or whose NFC quick check is not Yes
-- read from the generated file itself, starters that have compositions, and seeded segments built from them."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "tokenizers_amd", "csrc", "nfc_tables.inc")
_cache = {}


def tables():
    """(active code points, {cp: flags}, decomposition rows, composition rows) of nfc_tables.inc"""
    if "t" not in _cache:
        flags, decomp, comp, sect = {}, {}, {}, None
        with open(INC) as fh:
            for line in fh:
                m = re.match(r"#ifdef NFC_WANT_(\w+)", line)
                if m:
                    sect = m.group(1)
                    continue
                if line.startswith("#endif"):
                    sect = None
                if sect is None or not line.startswith("{"):
                    continue
                v = [int(x, 0) for x in line.strip().strip("{},").split(",")]
                if sect == "RUNS":
                    for cp in range(v[0], v[1] + 1):
                        flags[cp] = v[2]
                elif sect == "DECOMP":
                    decomp[v[0]] = [x for x in v[1:] if x != 0x1FFFFF]
                else:
                    comp[(v[0], v[1])] = v[2]
        active = sorted(cp for cp, f in flags.items() if f & 0xBF and not 0xD800 <= cp < 0xE000)
        _cache["t"] = (active, flags, decomp, comp)
    return _cache["t"]


def scalars():
    return [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]


def composing_starters(k=300, seed=5):
    """starters that are the first of a primary composite (every k-th kind of them), plus the Hangul L / LV that compose by arithmetic"""
    _, flags, _, comp = tables()
    firsts = sorted({a for a, _ in comp if not flags.get(a, 0) & 0x3F})
    rng = random.Random(seed)
    pick = set(rng.sample(firsts, min(k, len(firsts)))) | {0x61, 0x41, 0x65, 0xE9, 0x1EA1, 0x3B1, 0x1F00, 0x915, 0x1100, 0xAC00, 0xAC1C, 0x9C7, 0xCC6, 0xCCA}
    return sorted(pick)


def random_segments(n, seed, lo=2, hi=12):
    """seeded strings of lo..hi chars from the active set and the bases they act on (a starter in front, mostly)"""
    active, _, _, _ = tables()
    bases = composing_starters()
    rng = random.Random(seed)
    marks = [cp for cp in active if cp < 0x3100 or rng.random() < 0.2]
    out = []
    for _ in range(n):
        k = rng.randint(lo, hi)
        cps = [rng.choice(bases) if (i == 0 and rng.random() < 0.8) or rng.random() < 0.15 else rng.choice(marks if rng.random() < 0.7 else active) for i in range(k)]
        out.append("".join(chr(c) for c in cps))
    return out


E, M3 = "e\u0301", "a\u0323\u0301\u0308"           # one mark that composes; three marks (two compose, in another order)
PADS = (13, 14, 15, 16, 61, 62, 63, 64, 4093, 4094, 4095, 4096)      # a segment straddling a 16-byte lane, a 64-byte word, a 4,096-byte workgroup
PROPER = ["\u0e20\u0e32\u0e29\u0e32\u0e44\u0e17\u0e22 \u0e01\u0e47 \u0e17\u0e35\u0e48\u0e19\u0e35\u0e48 \u0e19\u0e49\u0e33 \u0e1c\u0e39\u0e49", "\u0939\u093f\u0928\u094d\u0926\u0940 \u0915\u094d\u0937\u0924\u094d\u0930\u093f\u092f \u0935\u093f\u0926\u094d\u092f\u093e", "\u0645\u064e\u0631\u0652\u062d\u064e\u0628\u064b\u0627 \u0628\u0650\u0643\u064f\u0645\u0652 \u0643\u0650\u062a\u064e\u0627\u0628\u064c", "\u05e2\u05b4\u05d1\u05b0\u05e8\u05b4\u05d9\u05ea"]      # marks in canonical order, all Quick_Check = Yes


def straddle_docs():
    return [("x" * p) + E + " y" for p in PADS] + [("x" * p) + M3 + "z" for p in PADS]


def edge_docs():
    """what the kernels can get wrong at the smallest places: see tests/test_nfc_gpu.py"""
    marks30 = "".join(chr(0x300 + (7 * k) % 0x30) for k in range(30))
    d = straddle_docs() + ["x" * 30 + E, "x" * 4094 + M3]      # (the last two END their document with the segment)
    d += [E, M3, E + "x", "x" + E, "x" + M3, "\u0301", "\u0301x", "", "abce", "\u0301xyz", "abc\u1100", "\u1161\u11a8 x"]      # ("abce" | mark: must not compose)
    d += ["a\u0301\u0301", "a\u0323\u0301", "a\u0301\u0323", "\u0958", "x\u0958y", "\u212b", "x\u212by", "\u0344", "a\u0344", "\U0001D15E", "\U0001D15E\U0001D15E x"]
    d += ["\u1100\u1161\u11a8", "\uac00\u11a8", "x" * 13 + "\uac00\u11a8", "x" * 14 + "\u1100\u1161\u11a8 z", "x" * 12 + "\u1100\u1161\u11a8\u11a8"]
    d += PROPER + ["a" + marks30 + " b", "\u0651\u064e", "\u0628\u0651\u064e \u0628\u064e\u0651", "\u00e9\u0323", "\u1e69 s\u0323\u0307 s\u0307\u0323"]
    d += ["a<|endoftext|>\u0301b", "e<|im_start|>\u0301<|im_end|>e\u0301", "<|endoftext|>", "x cafe\u0301 y", "caf\u00e9 au lait", "cafe\u0301 au lait", "xe\u0301e e\u0301 e", "cafe\u0301<|endoftext|>cafe\u0301",
          "plain ASCII text, nothing to do here at all", "caf\u00e9 na\u00efve r\u00e9sum\u00e9 Stra\u00dfe", "\u4e2d\u6587\u5b57\u7b26 and \u65e5\u672c\u8a9e", "\ud55c\uad6d\uc5b4 \ubb38\uc7a5", "emoji \U0001f600 \U0001f389", "\u0395\u03bb\u03bb\u03b7\u03bd\u03b9\u03ba\u03ac \u03ac \u03ac", "\u03a9 \u00c5 K"]
    return d
