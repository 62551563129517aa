#!/usr/bin/env python3
"""BLOOM's Split + ByteLevel(use_regex=false) (kernels/pretok_bloom.hip) on the C2 tokenizer and corpus of bench.py (GPT-2 byte-level
BPE, 50,257 vocab; 1 M synthetic lines) with ONLY the pre-tokenizer section swapped: the plain GPT-2 layout (C2 as it stands: the
yardstick, k_pretok_gpt2_seq), Digits in front of it (k_pretok_digits) and BLOOM's Sequence, on the same text with the same vocabulary,
in one session.  Per layout: the ids-only step and the char-offsets step (with word ids; the lead-byte mask rides in the lane kernel),
time and GB/s, and the per-stage HIP-event times (the pre-tokenizer's launch among them).  usage: python tools/bloom_perf.py [n_lines]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import tokenizers_amd as ta

n_lines = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
js_gpt2, n_types, _ = bench.load_config("c2")
bytelevel = json.loads(js_gpt2)["pre_tokenizer"]
assert bytelevel["type"] == "ByteLevel" and bytelevel["use_regex"] and not bytelevel["add_prefix_space"], bytelevel
BLOOM_PATTERN = " ?[^(\\s|[.,!?…。，、।۔،])]+"


def with_pretok(*members):
    d = json.loads(js_gpt2)
    d["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": list(members)}
    return json.dumps(d, ensure_ascii=False)


js_digits = with_pretok({"type": "Digits", "individual_digits": False}, bytelevel)
js_bloom = with_pretok({"type": "Split", "pattern": {"Regex": BLOOM_PATTERN}, "behavior": "Isolated", "invert": False}, dict(bytelevel, use_regex=False))

docs = bench.make_corpus("c2", n_lines, 100, 0, n_types)
stream = torch.cuda.current_stream().cuda_stream
buf, off = ta.pack_documents(docs)
d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
print(f"# {int(off[-1])} bytes, {len(docs)} documents")


def run(label, tok, offsets):
    enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), int(off[-1]), offsets=offsets, word_ids=offsets != "none", stream=stream)
    b = enc().sync()
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
    for _ in range(40):
        enc()
    enc().sync()
    tok.profile(False)
    st = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
    print(f"{label} offsets={offsets}: {int(off[-1]) / dt / 1e9:.1f} GB/s {dt * 1e3:.4f} ms a step (blocks of 20: {' '.join('%.4f' % (t * 1e3) for t in times)}), "
          f"{b.n_pretokens} pre-tokens, {b.n_tokens} tokens")
    print("   ", {k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004 or k.startswith("pretok")}, flush=True)


toks = [(label, ta.Tokenizer.from_str(js, device=0)) for label, js in (("GPT-2 layout (C2)     ", js_gpt2), ("Digits contiguous + it", js_digits), ("BLOOM's Split         ", js_bloom))]
for offsets in ("none", "char"):
    for rep in range(2):                                # (each layout twice a mode, alternating: the stage times' own spread)
        for label, tok in toks:
            run(label, tok, offsets)
