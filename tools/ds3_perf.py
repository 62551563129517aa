#!/usr/bin/env python3
"""The chained Split pre-tokenizer of DeepSeek-V3 / R1 (kernels/pretok_ds3.hip) on the C4 tokenizer and corpus of bench.py (Llama-3 style
Split + ByteLevel + BPE, 128,000 vocab; 1 M synthetic lines) with ONLY the pre-tokenizer section swapped for the chain of
tests/golden/ds3_chain.json.gz: ids-only step time and GB/s of the Llama-3 rule (C4 as it stands: the yardstick) and of the chain on the
same text, the per-stage HIP-event times of each (the pre-tokenizer's among them) and the share of documents the lane kernel handed to
the sequential matcher.  usage: python tools/ds3_perf.py [n_lines]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import tokenizers_amd as ta
from tests.helpers import load_tokenizer_json

n_lines = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
js_l3, n_types, _ = bench.load_config("c4")
d = json.loads(js_l3)
d["pre_tokenizer"] = json.loads(load_tokenizer_json("ds3_chain"))["pre_tokenizer"]
js_ds3 = json.dumps(d, ensure_ascii=False)
docs = bench.make_corpus("c4", n_lines, 100, 0, n_types)
stream = torch.cuda.current_stream().cuda_stream
buf, off = ta.pack_documents(docs)
d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()


def run(label, js, offsets):
    tok = ta.Tokenizer.from_str(js, device=0)
    enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), int(off[-1]), offsets=offsets, word_ids=offsets != "none", stream=stream)
    b = enc().sync()
    slow = tok.queue_sizes()["pretok_slow_docs"]
    for _ in range(3):
        enc().sync()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                                  # three timed blocks of 20 steps: the spread rides along
        t0 = time.perf_counter()
        for _ in range(20):
            r = enc()
        r.sync()
        times.append((time.perf_counter() - t0) / 20)
    dt = sorted(times)[1]
    tok.profile(True)
    for _ in range(10):
        enc()
    enc().sync()
    tok.profile(False)
    st = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
    print(f"{label} offsets={offsets}: {int(off[-1]) / dt / 1e9:.1f} GB/s {dt * 1e3:.4f} ms a step (blocks of 20: {' '.join('%.4f' % (t * 1e3) for t in times)}), "
          f"{int(off[-1])} bytes, {len(docs)} documents, {b.n_pretokens} pre-tokens, {b.n_tokens} tokens; sequential tier: {slow} documents ({100.0 * slow / len(docs):.3f} %)")
    print("   ", {k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004 or k.startswith("pretok")})


for offsets in ("none", "char"):
    run("Llama-3 rule (C4)  ", js_l3, offsets)
    run("chained Split (DS3)", js_ds3, offsets)
