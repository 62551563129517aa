#!/usr/bin/env python3
"""The NFKC normalizer (kernels/nfkc.hip, the K mode of csrc/nfc_core.hpp) in front of the "▁" front: the ids-only step of the
nfkc_spm_bpe fixture on 100,000 synthetic lines (12 MB: the normalizer's bound, 33 x the text through the front and the added tokens'
match list on top, refuses this fixture's batches above about 55 MB -- DESIGN sections 4 and 8), device entry.  Legs, alternating in one process:
    none   the same file with `normalizer: null` -- the path the "▁" front had before (run twice: the session's own spread)
    nfkc   the fixture as it is: count, scan, write in K mode for every batch, then the front over the normalized text
on the corpus as it is (ASCII) and with 1 % of the documents holding fullwidth / ligature chars.
Prints the step times, the per-stage HIP-event times and both ratios.  A 1 % sample is checked against the wheel where it is importable.
usage: python tools/nfkc_perf.py [n_lines]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokenizers_amd as ta
from oracle import synth
from tests.helpers import load_tokenizer_json

try:
    import tokenizers as ref
except ImportError:
    ref = None

n_lines = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
JS_NFKC = load_tokenizer_json("nfkc_spm_bpe")
_d = json.loads(JS_NFKC)
_d["normalizer"] = None
_d["added_tokens"] = [dict(a, normalized=False) for a in _d["added_tokens"]]
JS_NONE = json.dumps(_d, ensure_ascii=False)
LEGS = [("none", JS_NONE), ("nfkc", JS_NFKC), ("none again", JS_NONE)]
docs = synth.gen_lines(n_lines, text_seed=100)
WIDE = {"a": "\uff41", "e": "\uff45", "o": "\uff4f", "t": "\uff54", "1": "\uff11"}


def widen(x):
    """fullwidth letters and digits, the fi / fl ligatures"""
    return "".join(WIDE.get(c, c) for c in x.replace("fi", "\ufb01").replace("fl", "\ufb02"))


mixed = [widen(x) if i % 100 == 0 else x for i, x in enumerate(docs)]      # 1 % of the documents
stream = torch.cuda.current_stream().cuda_stream


def run(label, js, lines):
    buf, off = ta.pack_documents(lines)
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    tok = ta.Tokenizer.from_str(js, device=0)
    enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(lines), int(off[-1]), stream=stream)
    b = enc().sync()
    checked = "unchecked (no wheel)"
    if ref is not None:
        ids, to = b.ids_tensor().cpu().numpy().view(np.uint32), b.tok_offsets_tensor().cpu().numpy()
        idx = list(range(0, len(lines), 100))
        exp = ref.Tokenizer.from_str(js).encode_batch([lines[i] for i in idx], add_special_tokens=False)
        for k, i in enumerate(idx):
            assert ids[to[i]:to[i + 1]].tolist() == exp[k].ids, lines[i]
        checked = "1 % sample == wheel"
    for _ in range(3):
        enc().sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        r = enc()
    r.sync()
    dt = (time.perf_counter() - t0) / 20
    tok.profile(True)
    for _ in range(10):
        enc()
    enc().sync()
    tok.profile(False)
    st = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
    print(f"{label:11s}: {int(off[-1]) / dt / 1e9:.1f} GB/s {dt * 1e3:.4f} ms a step, {int(off[-1])} bytes, {b.n_tokens} tokens, {checked}")
    print("   ", {k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004 or "normalize" in k})
    return dt


for corpus, lines in (("corpus as it is (ASCII)", docs), ("1 % of the documents fullwidth / ligatures", mixed)):
    print(f"---- {corpus}")
    t = {label: run(label, js, lines) for label, js in LEGS}
    spread = abs(t["none"] - t["none again"])
    print(f"    spread of the session (none twice) {spread * 1e3:.4f} ms; nfkc - none {(t['nfkc'] - t['none']) * 1e3:+.4f} ms; nfkc / none {t['nfkc'] / t['none']:.2f} x")
