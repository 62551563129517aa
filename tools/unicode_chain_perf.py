#!/usr/bin/env python3
"""The NFD / Lowercase / StripAccents normalizer chains on the C3 tokenizer and corpus of bench.py (BertPreTokenizer + WordPiece, 30,522
vocab; 1 M synthetic lines).  Legs, alternating in one session:
    bert   BertNormalizer(clean_text=false, handle_chinese_chars=false), lowercase + strip_accents on  (run twice: the session's own spread)
    nls    Sequence[NFD, Lowercase, StripAccents], same vocabulary: the same two kernels over the chain's tables, no reorder pass
    nl     Sequence[NFD, Lowercase]: the NFC normalizer's kernels in their NFD mode (the general path for every batch)
each ids-only and with char offsets + word ids, on the corpus as it is and with 1 % of the documents accented.
Prints the step times and the per-stage HIP-event times.  usage: python tools/unicode_chain_perf.py [n_lines]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import tokenizers_amd as ta

n_lines = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
js_c3, n_types, _ = bench.load_config("c3")


def with_normalizer(norm):
    d = json.loads(js_c3)
    d["normalizer"] = norm
    return json.dumps(d, ensure_ascii=False)


MEMBER = {"N": {"type": "NFD"}, "L": {"type": "Lowercase"}, "S": {"type": "StripAccents"}}
JS_BERT = with_normalizer({"type": "BertNormalizer", "clean_text": False, "handle_chinese_chars": False, "strip_accents": True, "lowercase": True})
LEGS = [("bert", JS_BERT),
        ("nls", with_normalizer({"type": "Sequence", "normalizers": [MEMBER[c] for c in "NLS"]})),
        ("nl", with_normalizer({"type": "Sequence", "normalizers": [MEMBER[c] for c in "NL"]})),
        ("bert again", JS_BERT)]
docs = bench.make_corpus("c3", n_lines, 100, 0, n_types)
accents = {"a": "\u00e1", "e": "\u00e9", "o": "\u00f6", "u": "\u00fc", "n": "\u00f1"}
accented = [("".join(accents.get(c, c) for c in x) if i % 100 == 0 else x) for i, x in enumerate(docs)]      # 1 % of the documents accented
stream = torch.cuda.current_stream().cuda_stream


def run(label, js, lines, offsets):
    buf, off = ta.pack_documents(lines)
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    tok = ta.Tokenizer.from_str(js, device=0)
    enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(lines), int(off[-1]), offsets=offsets, word_ids=offsets != "none", stream=stream)
    b = enc().sync()
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
    print(f"{label:11s} offsets={offsets}: {int(off[-1]) / dt / 1e9:.1f} GB/s {dt * 1e3:.4f} ms a step, {int(off[-1])} bytes, {b.n_tokens} tokens")
    print("   ", {k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004 or "normalize" in k})
    return dt


for corpus, lines in (("corpus as it is", docs), ("1 % accented", accented)):
    for offsets in ("none", "char"):
        print(f"---- {corpus}, offsets={offsets}")
        t = {}
        for label, js in LEGS:
            t[label] = run(label, js, lines, offsets)
        spread = abs(t["bert"] - t["bert again"])
        print(f"    spread of the session (bert twice) {spread * 1e3:.4f} ms; nls - bert {(t['nls'] - t['bert']) * 1e3:+.4f} ms; nl - bert {(t['nl'] - t['bert']) * 1e3:+.4f} ms")
