#!/usr/bin/env python3
"""Unigram (kernels/unigram.hip) on the bench's synthetic lines: step time of the device path with fixture unigram_ms, ids only and with char
offsets + word ids, per kernel by HIP events -- next to two yardsticks of the same session: the reference wheel's encode_batch on this
machine's CPUs (its Rayon pool, sized by RAYON_NUM_THREADS or the CPUs the process may use) and spm_bpe_llama2 through this library on the
same text (the same front, lookup and compaction: the difference is the model kernels).  A 1 % sample is checked against the wheel.
Prints the report and, with --out FILE, writes it there too.  usage: python tools/unigram_perf.py [--lines N] [--out FILE]"""
import argparse
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

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


docs = synth.gen_lines(args.lines, text_seed=100)
buf, off = ta.pack_documents(docs)
n_bytes = int(off[-1])
d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
stream = torch.cuda.current_stream().cuda_stream
say(f"corpus: {len(docs)} synthetic lines, {n_bytes / 1e6:.1f} MB, device entry (inputs and outputs resident in HBM)")
gbs = {}
for name in ("unigram_ms", "spm_bpe_llama2"):
    js = load_tokenizer_json(name)
    tok = ta.Tokenizer.from_str(js, device=0)
    for label, kw in (("ids only", {}), ("char offsets + word ids", {"offsets": "char", "word_ids": True})):
        enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), n_bytes, stream=stream, **kw)
        b = enc().sync()
        checked = "unchecked (no wheel)"
        if ref is not None and not kw:
            ids, to = b.ids_tensor().cpu().numpy().view(np.uint32), b.tok_offsets_tensor().cpu().numpy()
            idx = list(range(0, len(docs), 100))
            exp = ref.Tokenizer.from_str(js).encode_batch([docs[i] for i in idx], add_special_tokens=False)
            for k, i in enumerate(idx):
                assert ids[to[i]:to[i + 1]].tolist() == exp[k].ids, docs[i]
            checked = "1 % sample == wheel"
        for _ in range(3):
            enc()
        torch.cuda.synchronize()
        steps = []
        for _ in range(3):                                   # the median of three blocks of 20 steps
            t0 = time.perf_counter()
            for _ in range(20):
                r = enc()
            r.sync()
            steps.append((time.perf_counter() - t0) / 20)
        dt = sorted(steps)[1]
        tok.profile(True)
        for _ in range(10):
            enc()
        enc().sync()
        tok.profile(False)
        st = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
        gbs[(name, label)] = n_bytes / dt / 1e9
        say(f"{name}, {label}: {n_bytes / dt / 1e9:.2f} GB/s, {dt * 1e3:.3f} ms a step ({', '.join('%.3f' % (s * 1e3) for s in steps)}), {b.n_tokens} tokens, "
            f"{b.n_pretokens} pre-tokens, {checked}")
        say("    HIP events, ms a launch: " + str({k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004}))
        if name == "unigram_ms":
            model = sum(v for k, v in st.items() if k.startswith("unigram"))
            say(f"    the Unigram launches: {model:.4f} ms = {model / (dt * 1e3) * 100:.1f} % of the step; queues {tok.queue_sizes()}")
if ref is not None:
    w = ref.Tokenizer.from_str(load_tokenizer_json("unigram_ms"))
    sub = docs[:max(1, len(docs) // 10)]                     # a tenth of the corpus: the wheel takes seconds for it
    nb = sum(len(d.encode("utf-8")) for d in sub)
    w.encode_batch(sub[:1000], add_special_tokens=False)
    t0 = time.perf_counter()
    w.encode_batch(sub, add_special_tokens=False)
    dt = time.perf_counter() - t0
    cpus = len(os.sched_getaffinity(0))
    wheel = nb / dt / 1e9
    say(f"reference wheel tokenizers=={ref.__version__}, encode_batch of unigram_ms on {nb / 1e6:.1f} MB of the same text: {wheel:.4f} GB/s "
        f"(RAYON_NUM_THREADS={os.environ.get('RAYON_NUM_THREADS', 'unset')}, {cpus} CPUs in the affinity mask)")
    ok = gbs[("unigram_ms", "ids only")] > wheel and gbs[("unigram_ms", "char offsets + word ids")] > wheel
    say(f"faster than the wheel: {'yes' if ok else 'NO'} ({gbs[('unigram_ms', 'char offsets + word ids')] / wheel:.0f} x with offsets, {gbs[('unigram_ms', 'ids only')] / wheel:.0f} x ids only)")
    assert ok
if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
