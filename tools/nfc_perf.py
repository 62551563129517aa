#!/usr/bin/env python3
"""The NFC normalizer (kernels/nfc.hip) on the C4 tokenizer and corpus of bench.py (Llama-3 style Split + ByteLevel + BPE, 128,000 vocab;
1 M synthetic lines): step time with and without the `"normalizer": {"type": "NFC"}` line, ids-only and with char offsets + word ids --
the all-NFC corpus runs over the text as it came behind k_nfc_check, so the two should differ by that kernel's time alone -- and a corpus
with 1 % of the documents decomposed, run with TKAMD_NO_SPECULATION so that every timed step takes the normalizer's kernels.
Prints the step times, the per-stage HIP-event times and the speculation counters.  usage: python tools/nfc_perf.py [n_lines]"""
import json
import os
import sys
import time
import unicodedata

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import tokenizers_amd as ta

n_lines = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
js_plain, n_types, _ = bench.load_config("c4")
d = json.loads(js_plain)
assert not d.get("normalizer")
d["normalizer"] = {"type": "NFC"}
js_nfc = json.dumps(d, ensure_ascii=False)
docs = bench.make_corpus("c4", n_lines, 100, 0, n_types)
accents = {"a": "á", "e": "é", "o": "ö", "u": "ü", "n": "ñ"}
mixed = [("".join(accents.get(c, c) for c in x) if i % 100 == 0 else x) for i, x in enumerate(docs)]      # 1 % of the documents decomposed
assert all(unicodedata.normalize("NFC", x) == x for x in docs[:2000])
stream = torch.cuda.current_stream().cuda_stream


def run(label, js, lines, offsets, outright=False):
    buf, off = ta.pack_documents(lines)
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    tok = ta.Tokenizer.from_str(js, device=0)
    enc = lambda: tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(lines), int(off[-1]), offsets=offsets, word_ids=offsets != "none", stream=stream, unsynced=outright)
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
    q = tok.queue_sizes()
    print(f"{label} offsets={offsets}: {int(off[-1]) / dt / 1e9:.1f} GB/s {dt * 1e3:.4f} ms a step, {int(off[-1])} bytes, {b.n_tokens} tokens; "
          f"nfc_reruns {q['nfc_reruns']} nfc_spec_pause {q['nfc_spec_pause']}")
    print("   ", {k: v for k, v in sorted(st.items(), key=lambda kv: -kv[1]) if v >= 0.004 or k.startswith("nfc")})
    return b.n_tokens


for offsets in ("none", "char"):
    a = run("no normalizer       ", js_plain, docs, offsets)
    b = run("NFC, all-NFC text   ", js_nfc, docs, offsets)
    assert a == b
    run("NFC, 1 % decomposed ", js_nfc, mixed, offsets, outright=True)      # (every step through the normalizer's kernels: no pause to run out)
