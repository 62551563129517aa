#!/usr/bin/env python3
"""Generates tokenizers_amd/csrc/nfc_tables.inc: the data of the NFC normalizer (csrc/nfc_core.hpp, kernels/nfc.hip), probed from the
REFERENCE wheel -- tokenizers.normalizers.NFC / NFD normalize_str over every scalar value.

Per code point (one byte of a 2-stage table, emitted as runs):
    bits 0..5  rank of the canonical combining class among the classes in use (0 = class 0; ranks keep the classes' order, and the
               order is all the canonical ordering and the blocking rule ask of a class)
    bit 6      DECOMPOSES: the full canonical decomposition (NFD) is not the char itself
    bit 7      NFC_Quick_Check is not Yes (No: NFC changes the char alone; Maybe: the second char of a primary composite, a Hangul V / T)
A char is ACTIVE -- it may change, move or compose behind what stands in front of it -- when its class is not 0 or bit 7 is set.
The full canonical decomposition of every char that has one (<= 4 code points; Hangul syllables are arithmetic and absent), and the
primary composites (first, second) -> composite (composition exclusions are simply absent; Hangul is arithmetic).

Where the classes come from: the wheel offers no class lookup, so the candidate is CPython's unicodedata, and the wheel is then asked,
scalar by scalar, whether it orders each char against two probe marks exactly as that class says (NFD of "U+0345 c" and of
"c U+0334": classes 240 and 1, the highest and the lowest) and, per class in use, whether neighbours in class order swap.  Any
disagreement stops the generator.  The same holds for the single-scalar NFC forms (unicodedata as the cross-check, the wheel as the
source)."""
import os
import sys
import unicodedata

from tokenizers import normalizers
import tokenizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tokenizers_amd", "csrc", "nfc_tables.inc")
S_BASE, L_BASE, V_BASE, T_BASE, L_N, V_N, T_N = 0xAC00, 0x1100, 0x1161, 0x11A7, 19, 21, 28
S_N = L_N * V_N * T_N


def scalars():
    for cp in range(0x110000):
        if not 0xD800 <= cp < 0xE000:
            yield cp


def main():
    nfc, nfd = normalizers.NFC().normalize_str, normalizers.NFD().normalize_str
    decomp, qc_no, disagree, nfd_only = {}, set(), 0, []
    for cp in scalars():
        c = chr(cp)
        d = nfd(c)
        if d != c:
            decomp[cp] = [ord(x) for x in d]
        n = nfc(c)
        if n != c:
            qc_no.add(cp)
        if n != unicodedata.normalize("NFC", c):
            disagree += 1
        elif d != unicodedata.normalize("NFD", c):
            nfd_only.append(cp)                             # (a decomposition the wheel's older tables lack: the wheel is the source)
    assert disagree == 0, f"{disagree} scalars: the wheel and unicodedata {unicodedata.unidata_version} disagree on NFC"
    assert all(len(v) <= 4 for v in decomp.values())
    for cp, v in decomp.items():                        # the 3x bound of the X text (UTF-8 bytes)
        assert sum(len(chr(x).encode()) for x in v) <= 3 * len(chr(cp).encode()), hex(cp)
    # ---- classes: asked of the wheel.  A char is a non-starter if NFD moves it across one of two probe marks (U+0345: class 240, the
    # highest; U+0334: class 1, the lowest); its class is then found among the classes in use by which representatives it swaps with
    # (c r -> r c exactly when class(c) > class(r)), and confirmed by not swapping with its own class's representative either way.
    # unicodedata names the candidates for the representatives and is the cross-check afterwards.
    hi, lo = "\u0345", "\u0334"
    rep = {}
    for cp in scalars():
        k = unicodedata.combining(chr(cp))
        if k and k not in rep and cp not in decomp and (nfd(hi + chr(cp)) == chr(cp) + hi or nfd(chr(cp) + lo) == lo + chr(cp) or cp in (0x345, 0x334)):
            rep[k] = chr(cp)
    classes = sorted(rep)
    assert classes[0] == 1 and classes[-1] == 240 and len(classes) < 64, classes
    for a, b in zip(classes, classes[1:]):                  # neighbours in class order: b a -> a b, a b stays
        assert nfd(rep[b] + rep[a]) == rep[a] + rep[b] and nfd(rep[a] + rep[b]) == rep[a] + rep[b], (a, b)
    rank = {0: 0}
    rank.update({k: i + 1 for i, k in enumerate(classes)})
    ccc, newer = {}, 0
    for cp in scalars():
        if cp in decomp:
            continue                                        # (its pieces are scalars of their own)
        c = chr(cp)
        if cp in (0x345, 0x334) or nfd(hi + c) == c + hi or nfd(c + lo) == lo + c:
            below = [a for a in classes if nfd(c + rep[a]) == rep[a] + c and c != rep[a]]
            k = classes[len(below)]
            assert below == classes[:len(below)] and nfd(c + rep[k]) == c + rep[k] and nfd(rep[k] + c) == rep[k] + c, hex(cp)
            ccc[cp] = k
        if ccc.get(cp, 0) != unicodedata.combining(c):
            assert cp not in ccc, hex(cp)                   # (the only way to differ: a mark newer than the wheel's tables, class 0 there)
            newer += 1
    # ---- primary composites: the one-step canonical pairs the wheel composes back
    comp = {}
    for cp in decomp:
        if S_BASE <= cp < S_BASE + S_N:
            continue
        f = unicodedata.decomposition(chr(cp)).split()
        if len(f) != 2 or f[0].startswith("<"):
            continue
        a, b = int(f[0], 16), int(f[1], 16)
        if cp in qc_no:                                     # an exclusion: never composed
            assert nfc(chr(a) + chr(b)) != chr(cp), hex(cp)
            continue
        assert nfc(chr(a) + chr(b)) == chr(cp), hex(cp)
        assert (a, b) not in comp
        comp[(a, b)] = cp
    seconds = {b for _, b in comp} | set(range(V_BASE, V_BASE + V_N)) | set(range(T_BASE + 1, T_BASE + T_N))
    assert min(b for _, b in comp) >= 0x300                 # (the pair keys never meet the decomposition keys (cp, 0 / 1) in the one table)
    flags = bytearray(0x110000)
    for cp in scalars():
        k = ccc.get(cp, 0)
        f = rank[k]
        if cp in decomp:
            f |= 0x40
        if cp in qc_no or cp in seconds:
            f |= 0x80
        flags[cp] = f
    for cp in range(S_BASE, S_BASE + S_N):                  # Hangul syllables: arithmetic on the device
        d = decomp.pop(cp)
        s = cp - S_BASE
        exp = [L_BASE + s // (V_N * T_N), V_BASE + (s % (V_N * T_N)) // T_N] + ([T_BASE + s % T_N] if s % T_N else [])
        assert d == exp, hex(cp)
    runs, cp = [], 0
    while cp < 0x110000:
        if flags[cp] == 0:
            cp += 1
            continue
        e = cp
        while e + 1 < 0x110000 and flags[e + 1] == flags[cp]:
            e += 1
        runs.append((cp, e, flags[cp]))
        cp = e + 1
    with open(OUT, "w") as fh:
        fh.write("// GENERATED by tools/gen_nfc_tables.py -- do not edit.\n")
        fh.write(f"// Source: probing the reference wheel tokenizers=={tokenizers.__version__} (normalizers NFC / NFD normalize_str over every scalar value;\n")
        fh.write(f"// cross-checked against unicodedata {unicodedata.unidata_version}: 0 of 1,112,064 scalars disagree, {len(qc_no)} change under NFC;\n")
        fh.write("// NFD differs on " + (", ".join("U+%04X" % c for c in nfd_only) or "none") + ": the wheel's form is taken)\n")
        fh.write("// runs: first, last, flags = rank of the canonical combining class (bits 0..5) | 64 DECOMPOSES | 128 NFC_QC != Yes\n")
        fh.write(f"// classes: from the wheel's own ordering of every scalar against probe marks; {newer} marks unicodedata knows are class 0 to the wheel\n")
        fh.write("// classes by rank: 0, " + ", ".join(str(k) for k in classes) + "\n")
        fh.write("// decomp: cp, then its full canonical decomposition, 0x1FFFFF-filled to four (Hangul syllables absent: arithmetic)\n")
        fh.write("// comp: first, second, primary composite (exclusions absent; Hangul absent: arithmetic)\n")
        fh.write(f"#define NFC_N_RUNS {len(runs)}\n#define NFC_N_DECOMP {len(decomp)}\n#define NFC_N_COMP {len(comp)}\n")
        fh.write("#ifdef NFC_WANT_RUNS\n")
        for a, b, f in runs:
            fh.write("{0x%X,0x%X,%d},\n" % (a, b, f))
        fh.write("#endif\n#ifdef NFC_WANT_DECOMP\n")
        for cp in sorted(decomp):
            v = decomp[cp] + [0x1FFFFF] * (4 - len(decomp[cp]))
            fh.write("{0x%X,0x%X,0x%X,0x%X,0x%X},\n" % (cp, *v))
        fh.write("#endif\n#ifdef NFC_WANT_COMP\n")
        for (a, b) in sorted(comp):
            fh.write("{0x%X,0x%X,0x%X},\n" % (a, b, comp[(a, b)]))
        fh.write("#endif\n")
    print("runs", len(runs), "decomp", len(decomp), "comp", len(comp), "classes", len(classes), "->", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    sys.exit(main())
