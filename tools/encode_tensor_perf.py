#!/usr/bin/env python3
"""Encode into padded [B, L] tensors on the device (Tokenizer.encode_tensor, kernels/dense.hip), measured in one session: the C2 tokenizer
(GPT-2 byte-level BPE, 50,257 vocab) with enable_truncation(128) and enable_padding(length=128) over B = 256, 4,096 and 65,536 corpus lines
of bench.py's C2.  Behind a warm-up, every number the median of REPS runs (each run in brackets):

 1. the dense stage alone -- the `dense_rows` profile stage, and the device step with the stage (tkamd_encode_batch_device_dense over text in
    HBM, HIP events) less the same step without it (tkamd_encode_batch_device with TKAMD_NO_SPECULATION), both on this build -- next to the
    time its traffic, B x L x (4 + 8 x outputs) bytes, takes at the 3.3 TB/s one read of the text reaches here (profiles/nfc_perf.txt);
 2. encode_tensor(list[str]) against the route without it: encode_batch_csr, padded input_ids / attention_mask built in numpy, one
    torch.from_numpy(...).to(device) each -- run on this build and, with --parent DIR (a built checkout of the commit before the dense
    stage), in a process of that checkout -- and against the wheel's encode_batch with the same numpy / torch step on the host's cores;
 3. encode_tensor over text already in HBM against encode_batch_device + sync() + the same masks built with torch ops from pad_counts.

usage: python tools/encode_tensor_perf.py [out.txt] [--parent DIR]   (default profiles/encode_tensor_perf.txt)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ROUTE_ONLY = "--host-route-only" in sys.argv          # (the child run inside --parent's checkout: sys.path[0] is that checkout)
if not HOST_ROUTE_ONLY:
    sys.path.insert(0, ROOT)
import numpy as np
import torch

L, REPS, WARM = 128, 7, 2
SIZES = (256, 4096, 65536)


def med(xs):
    return statistics.median(xs), "[" + " ".join("%.3f" % x for x in xs) + "]"


def corpus(n):
    import bench
    _, n_types, _ = bench.load_config("c2")
    return bench.make_corpus("c2", n, 100, 0, n_types)


def tokenizer_json():
    import bench
    d = json.loads(bench.load_config("c2")[0])
    d["truncation"] = {"direction": "Right", "max_length": L, "strategy": "LongestFirst", "stride": 0}
    d["padding"] = {"strategy": {"Fixed": L}, "direction": "Right", "pad_to_multiple_of": None, "pad_id": 0, "pad_type_id": 0, "pad_token": "<pad>"}
    return json.dumps(d)


def timed(fn, reps=REPS, warm=WARM):
    """wall milliseconds of fn() + a device synchronisation, per run"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def host_route(tok, docs):
    """what a caller does without encode_tensor: the CSR to the host, padded rows and the mask in numpy, both up again"""
    be = tok.encode_batch_csr(docs, add_special_tokens=True)
    ids = be.ids.reshape(len(docs), L).astype(np.int64)
    mask = (np.arange(L)[None, :] < (L - be.pad_counts.astype(np.int64))[:, None]).astype(np.int64)
    return torch.from_numpy(ids).to("cuda"), torch.from_numpy(mask).to("cuda")


def host_route_times():
    import tokenizers_amd as ta
    tok = ta.Tokenizer.from_str(tokenizer_json(), device=0)
    out = {}
    for B in SIZES:
        docs = corpus(B)
        out[B] = timed(lambda: host_route(tok, docs))
    return out


if HOST_ROUTE_ONLY:
    # (PYTHONPATH names the checkout: its tokenizers_amd, bench.py and corpus)
    print("HOST_ROUTE " + json.dumps(host_route_times()))
    sys.exit(0)

import tokenizers

import tokenizers_amd as ta
from tokenizers_amd import _lib

args = [a for a in sys.argv[1:] if not a.startswith("--")]
parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
if parent in args:
    args.remove(parent)
out_path = args[0] if args else os.path.join(ROOT, "profiles", "encode_tensor_perf.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


js = tokenizer_json()
tok = ta.Tokenizer.from_str(js, device=0)
ref = tokenizers.Tokenizer.from_str(js)
assert tok.dense_width() == L
say(f"# encode_tensor: C2 tokenizer, truncation {L}, Fixed padding {L}, {_lib.load().tkamd_version().decode()}, wheel {tokenizers.__version__}, "
    f"medians of {REPS} behind {WARM} warm-up runs, milliseconds")
parent_times = None
if parent:
    env = dict(os.environ, PYTHONPATH=os.path.abspath(parent))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-route-only"], cwd=os.path.abspath(parent), env=env, capture_output=True, text=True, timeout=1500)
    got = [l for l in r.stdout.splitlines() if l.startswith("HOST_ROUTE ")]
    assert got, r.stdout[-2000:] + r.stderr[-2000:]
    parent_times = {int(k): v for k, v in json.loads(got[-1][len("HOST_ROUTE "):]).items()}
stream = torch.cuda.current_stream().cuda_stream
for B in SIZES:
    docs = corpus(B)
    buf, off = ta.pack_documents(docs)
    n_bytes = int(off[-1])
    d_text, d_off = torch.from_numpy(np.array(buf)).cuda(), torch.from_numpy(np.array(off)).cuda()
    say(f"## B = {B}: {n_bytes / 1e6:.2f} MB of text, [B, L] = [{B}, {L}]")
    # ---- 1. the stage alone ----
    for n_out, keys in ((2, ("input_ids", "attention_mask")), (4, ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask"))):
        outs = {k: torch.empty((B, L), dtype=torch.int64, device="cuda") for k in keys}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}

        def dense():
            tok.encode_batch_device_dense(d_text.data_ptr(), d_off.data_ptr(), B, n_bytes, ptrs, L, stream=stream)

        def plain():
            res = _lib.DeviceResult()
            _lib.check(tok._lib.tkamd_encode_batch_device(tok._h, d_text.data_ptr(), d_off.data_ptr(), B, n_bytes, _lib.ADD_SPECIAL | _lib.NO_SPECULATION, stream, res))

        def events(fn):
            for _ in range(WARM):
                fn()
            ts = []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            return ts
        t_dense, t_plain = events(dense), events(plain)
        tok.profile(True)
        tok.profile_read()
        for _ in range(REPS):
            dense()
            tok._lib.tkamd_device_sync(tok._h, stream, None, None)
        prof = tok.profile_read()
        tok.profile(False)
        stage_ms = prof["dense_rows"][0] / max(prof["dense_rows"][1], 1)
        traffic = B * L * (4 + 8 * n_out)
        floor_ms = traffic / 3.3e12 * 1e3
        (md, sd), (mp, sp) = med(t_dense), med(t_plain)
        say(f"stage, {n_out} outputs: dense_rows profile stage {stage_ms:.4f} (mean of {prof['dense_rows'][1]} launches); device step with it {md:.3f} {sd}, "
            f"without {mp:.3f} {sp}, difference {md - mp:.3f}; traffic {traffic / 1e6:.2f} MB = {floor_ms:.4f} at 3.3 TB/s: the stage takes "
            f"{stage_ms / floor_ms:.1f} x that")
    # ---- 2. list[str] in, tensors on the device out ----
    t_new = timed(lambda: tok.encode_tensor(docs, return_token_type_ids=False))
    t_old = timed(lambda: host_route(tok, docs))

    def wheel_route():
        encs = ref.encode_batch(docs, add_special_tokens=True)
        ids = np.array([e.ids for e in encs], dtype=np.int64)
        mask = np.array([e.attention_mask for e in encs], dtype=np.int64)
        return torch.from_numpy(ids).to("cuda"), torch.from_numpy(mask).to("cuda")
    t_ref = timed(wheel_route, reps=3, warm=1)
    a, b = tok.encode_tensor(docs, return_token_type_ids=False), host_route(tok, docs)
    c = wheel_route()
    assert torch.equal(a["input_ids"], b[0]) and torch.equal(a["attention_mask"], b[1]) and torch.equal(a["input_ids"], c[0]) and torch.equal(a["attention_mask"], c[1])
    (mn, sn), (mo, so), (mr, sr) = med(t_new), med(t_old), med(t_ref)
    say(f"list[str]: encode_tensor {mn:.3f} {sn}; encode_batch_csr + numpy + 2 x to(device), this build {mo:.3f} {so} = {mo / mn:.2f} x"
        + (f"; the same on the parent commit {med(parent_times[B])[0]:.3f} {med(parent_times[B])[1]} = {med(parent_times[B])[0] / mn:.2f} x" if parent_times else "")
        + f"; wheel encode_batch + numpy + 2 x to(device) {mr:.3f} {sr} = {mr / mn:.2f} x")
    # ---- 3. text in HBM in ----
    text = torch.zeros(n_bytes + _lib.TEXT_PAD, dtype=torch.uint8, device="cuda")
    text[:n_bytes] = d_text[:n_bytes]

    def device_old():
        batch = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), B, n_bytes, stream=stream).sync()
        ids = batch.ids_tensor().view(B, L).to(torch.int64)
        pads = batch._tensor(batch._res.d_pad_counts, (B,), "<i4").to(torch.int64)
        return ids, (torch.arange(L, device="cuda")[None, :] < (L - pads)[:, None]).to(torch.int64)
    t_dnew = timed(lambda: tok.encode_tensor((text[:n_bytes], d_off), add_special_tokens=False, return_token_type_ids=False))
    t_dold = timed(device_old)
    a, b = tok.encode_tensor((text[:n_bytes], d_off), add_special_tokens=False, return_token_type_ids=False), device_old()
    torch.cuda.synchronize()
    assert torch.equal(a["input_ids"], b[0]) and torch.equal(a["attention_mask"], b[1])
    (mn, sn), (mo, so) = med(t_dnew), med(t_dold)
    say(f"text in HBM: encode_tensor {mn:.3f} {sn}; encode_batch_device + sync() + torch ops from pad_counts {mo:.3f} {so} = {mo / mn:.2f} x")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w", encoding="utf-8") as fh:
    fh.write("\n".join(lines) + "\n")
