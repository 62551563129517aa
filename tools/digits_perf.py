#!/usr/bin/env python3
"""Sequence[Digits, ByteLevel(use_regex=true)] of the StarCoder family (kernels/pretok_digits.hip) on the C2 tokenizer and corpus of
bench.py (GPT-2 byte-level BPE, 50,257 vocab; 1 M synthetic lines) with ONLY the pre-tokenizer section swapped: the plain GPT-2 layout
(C2 as it stands: the yardstick, k_pretok_gpt2_seq) and Digits in front of it, individual and contiguous, on the same text with the same
vocabulary, in one session.  Per layout: the ids-only step and the with-offsets steps (byte and char offsets with word ids), time and
GB/s, and the per-stage HIP-event times (the pre-tokenizer's launch among them).  usage: python tools/digits_perf.py [n_lines]"""
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


def with_digits(individual):
    d = json.loads(js_gpt2)
    d["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [{"type": "Digits", "individual_digits": individual}, bytelevel]}
    return json.dumps(d, ensure_ascii=False)


docs = bench.make_corpus("c2", n_lines, 100, 0, n_types)
stream = torch.cuda.current_stream().cuda_stream
buf, off = ta.pack_documents(docs)
d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
digit_bytes = sum(int((buf == c).sum()) for c in range(0x30, 0x3A))
print(f"# {int(off[-1])} bytes, {len(docs)} documents, {digit_bytes} ASCII digits ({100.0 * digit_bytes / int(off[-1]):.2f} % of the bytes)")


def run(label, js, offsets):
    tok = ta.Tokenizer.from_str(js, device=0)
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
    for _ in range(20):
        enc()
    enc().sync()
    tok.profile(False)
    st = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
    print(f"{label} offsets={offsets}: {int(off[-1]) / dt / 1e9:.1f} GB/s {dt * 1e3:.4f} ms a step (blocks of 20: {' '.join('%.4f' % (t * 1e3) for t in times)}), "
          f"{b.n_pretokens} pre-tokens, {b.n_tokens} tokens")
    print("   ", {k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004 or k.startswith("pretok")})


for offsets in ("none", "byte", "char"):
    run("GPT-2 layout (C2)     ", js_gpt2, offsets)
    run("Digits individual + it", with_digits(True), offsets)
    run("Digits contiguous + it", with_digits(False), offsets)
