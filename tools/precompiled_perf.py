#!/usr/bin/env python3
"""The Precompiled normalizer (kernels/precompiled.hip) in front of Unigram: step time of the XLM-R layout (fixture precompiled_xlmr, the
nmt_nfkc-like charsmap) per kernel by HIP events and in GB/s, ids only and with char offsets + word ids, on four texts -- the bench's
synthetic lines, the same with a char of the charsmap in about 1 % and in about 30 % of the 16-byte lanes, and a text without spaces --
next to the yardstick of the same session: the same vocabulary behind bare Metaspace WITHOUT the normalizer on the same text (what the
parent commit could already run).  A 1 % sample of every text is checked against the reference wheel where it imports.
Prints the report and, with --out FILE, writes it there too.  usage: python tools/precompiled_perf.py [--lines N] [--out FILE]"""
import argparse
import json
import os
import random
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

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=100_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def sprinkle(docs, every, seed):
    """a char the charsmap changes (or a tab) about every `every` bytes"""
    rng = random.Random(seed)
    odd = ["\u00e9", "\uff21", "\ufb03", "\t", "\u2122", "\u00a0", "e\u0301", "\u4e2d"]
    out = []
    for d in docs:
        parts, k = [], 0
        while k < len(d):
            step = max(1, int(rng.expovariate(1.0 / every)))
            parts.append(d[k:k + step])
            k += step
            if k < len(d):
                parts.append(rng.choice(odd))
        out.append("".join(parts))
    return out


def non_plain_share(buf):
    """the share of 16-byte lanes with a byte that is not ASCII or is a control (what keeps a lane of this charsmap from being copied)"""
    n = len(buf) // 16 * 16
    b = buf[:n].reshape(-1, 16)
    return float(((b >= 0x80) | (b < 0x20) | (b == 0x7F)).any(axis=1).mean())


base = synth.gen_lines(args.lines, text_seed=100)
texts = {"bench lines": base, "~1 % of the lanes": sprinkle(base, 1600, 1), "~30 % of the lanes": sprinkle(base, 45, 2),
         "no spaces": [d.replace(" ", "") for d in base]}
js = load_tokenizer_json("precompiled_xlmr")
d = json.loads(js)
d["normalizer"] = None
d["pre_tokenizer"] = d["pre_tokenizer"]["pretokenizers"][1]
files = {"precompiled_xlmr": js, "same vocabulary, bare Metaspace, no normalizer": json.dumps(d, ensure_ascii=False)}
stream = torch.cuda.current_stream().cuda_stream
for tname, docs in texts.items():
    buf, off = ta.pack_documents(docs)
    n_bytes = int(off[-1])
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    say(f"== {tname}: {len(docs)} lines, {n_bytes / 1e6:.1f} MB, {100 * non_plain_share(buf):.2f} % of the lanes not plain; device entry")
    step = {}
    for name, fjs in files.items():
        tok = ta.Tokenizer.from_str(fjs, device=0)
        for label, kw in (("ids only", {}), ("char offsets + word ids", {"offsets": "char", "word_ids": True})):
            enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), n_bytes, stream=stream, **kw)
            b = enc().sync()
            checked = "unchecked"
            if ref is not None and not kw:
                ids, to = b.ids_tensor().cpu().numpy().view(np.uint32), b.tok_offsets_tensor().cpu().numpy()
                idx = list(range(0, len(docs), 100))
                exp = ref.Tokenizer.from_str(fjs).encode_batch([docs[i] for i in idx], add_special_tokens=False)
                for k, i in enumerate(idx):
                    assert ids[to[i]:to[i + 1]].tolist() == exp[k].ids, docs[i]
                checked = "1 % sample == wheel"
            for _ in range(3):
                enc()
            torch.cuda.synchronize()
            steps = []
            for _ in range(3):                                   # the median of three blocks of 10 steps
                t0 = time.perf_counter()
                for _ in range(10):
                    r = enc()
                r.sync()
                steps.append((time.perf_counter() - t0) / 10)
            dt = sorted(steps)[1]
            tok.profile(True)
            for _ in range(5):
                enc()
            enc().sync()
            tok.profile(False)
            st = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
            step[(name, label)] = dt
            say(f"{name}, {label}: {n_bytes / dt / 1e9:.2f} GB/s, {dt * 1e3:.3f} ms a step ({', '.join('%.3f' % (s * 1e3) for s in steps)}), {b.n_tokens} tokens, {checked}")
            say("    HIP events, ms a launch: " + str({k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004}))
            if name == "precompiled_xlmr":
                pcn = st.get("precompiled_normalize", 0.0)
                say(f"    the normalizer's launches: {pcn:.4f} ms = {pcn / (dt * 1e3) * 100:.1f} % of the step, {n_bytes / max(pcn, 1e-9) / 1e6:.1f} GB/s of source text")
    for label in ("ids only", "char offsets + word ids"):
        a, y = step[("precompiled_xlmr", label)], step[("same vocabulary, bare Metaspace, no normalizer", label)]
        say(f"   {label}: {a / y:.2f} x the yardstick's step")
if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
