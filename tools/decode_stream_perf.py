#!/usr/bin/env python3
"""Streaming decode (Tokenizer.decode_stream, kernels/decode_stream.hip) against the reference wheel's DecodeStream, in one session: 256 and
4,096 streams stepped 128 times over ids encoded from the corpus lines of bench.py's C2 (GPT-2 byte-level BPE, 50,257 vocab).  Per stream
count: the time per step_tensor (ids in HBM, HIP events around the loop, behind a warm-up), the time per host step (ids up, strings down)
and the time per step of as many DecodeStream objects of the wheel on one host thread -- and, beside them, the same for a FUSED object
(decode_stream(fused=True): a step only enqueues): its step_tensor, a replayed graph of ONE captured fused step_tensor, and its host step.
Every number is the median of three runs (each run in brackets), with the ratios to the wheel.  The chunks of all of them are compared on
the way.
usage: python tools/decode_stream_perf.py [out.txt]   (default profiles/decode_stream_perf.txt)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import tokenizers
from tokenizers.decoders import DecodeStream

import bench
import tokenizers_amd as ta

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decode_stream_perf.txt")
N_STEPS, WARM, REPS = 128, 8, 3
js, n_types, _ = bench.load_config("c2")
tok = ta.Tokenizer.from_str(js, device=0)
ref = tokenizers.Tokenizer.from_str(js)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f"# decode_stream: {N_STEPS} steps a run, C2 tokenizer, {ta._lib.load().tkamd_version().decode()}, wheel {tokenizers.__version__}")
for n_streams in (256, 4096):
    need = n_streams * (N_STEPS + WARM)
    docs = bench.make_corpus("c2", max(2000, need // 12), 100, 0, n_types)
    flat = tok.encode_batch_fast(docs, add_special_tokens=False).ids.astype(np.int64)
    assert len(flat) >= need, (len(flat), need)
    ids = np.ascontiguousarray(flat[:need].reshape(n_streams, N_STEPS + WARM).T)       # [step, stream]: stream s reads on through its own lines
    d_ids = torch.from_numpy(ids).cuda()
    ds = tok.decode_stream(n_streams, skip_special_tokens=False)
    dsf = tok.decode_stream(n_streams, skip_special_tokens=False, fused=True)
    rows = ids.tolist()
    t_dev, t_host, t_ref, t_fdev, t_graph, t_fhost = [], [], [], [], [], []
    # one fused step captured once, behind a warm-up step on the capturing stream; a replay reads the ids the static tensor holds
    static_ids = d_ids[0].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dsf.step_tensor(static_ids)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_text, g_status = dsf.step_tensor(static_ids)
    for rep in range(REPS):                                 # the same 128 steps three times: the spread rides along
        # ids in HBM, text and status left there
        ds.reset()
        for j in range(WARM):
            ds.step_tensor(d_ids[j])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for j in range(WARM, WARM + N_STEPS):
            text, status = ds.step_tensor(d_ids[j])
        b.record()
        torch.cuda.synchronize()
        t_dev.append(a.elapsed_time(b) / N_STEPS)
        last_dev = text.to_strings()
        # the same, fused: the loop only enqueues
        dsf.reset()
        for j in range(WARM):
            dsf.step_tensor(d_ids[j])
        torch.cuda.synchronize()
        a.record()
        for j in range(WARM, WARM + N_STEPS):
            text, status = dsf.step_tensor(d_ids[j])
        b.record()
        torch.cuda.synchronize()
        t_fdev.append(a.elapsed_time(b) / N_STEPS)
        last_fdev = text.to_strings()
        # the captured fused step replayed, the ids copied into its static tensor on the device in front of every replay
        dsf.reset()
        for j in range(WARM):
            static_ids.copy_(d_ids[j])
            graph.replay()
        torch.cuda.synchronize()
        a.record()
        for j in range(WARM, WARM + N_STEPS):
            static_ids.copy_(d_ids[j])
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        t_graph.append(a.elapsed_time(b) / N_STEPS)
        last_graph = g_text.to_strings()
        # host ids in, strings out: fused (its only wait is the read)
        dsf.reset()
        for j in range(WARM):
            dsf.step(ids[j])
        t0 = time.perf_counter()
        for j in range(WARM, WARM + N_STEPS):
            got_f = dsf.step(ids[j])
        t_fhost.append((time.perf_counter() - t0) * 1e3 / N_STEPS)
        # host ids in, strings out
        ds.reset()
        for j in range(WARM):
            ds.step(ids[j])
        t0 = time.perf_counter()
        for j in range(WARM, WARM + N_STEPS):
            got = ds.step(ids[j])
        t_host.append((time.perf_counter() - t0) * 1e3 / N_STEPS)
        # the wheel: one DecodeStream a stream, one host thread
        ws = [DecodeStream(skip_special_tokens=False) for _ in range(n_streams)]
        for j in range(WARM):
            for s in range(n_streams):
                ws[s].step(ref, rows[j][s])
        t0 = time.perf_counter()
        for j in range(WARM, WARM + N_STEPS):
            row = rows[j]
            exp = [ws[s].step(ref, row[s]) for s in range(n_streams)]
        t_ref.append((time.perf_counter() - t0) * 1e3 / N_STEPS)
    assert got == exp and last_dev == [c or "" for c in exp], "the last step's chunks differ from the wheel's"
    assert got_f == exp and last_fdev == last_dev and last_graph == last_dev, "the fused step's chunks differ from the wheel's"
    fmt = lambda ts: f"{sorted(ts)[REPS // 2]:.4f} ms a step ({' '.join('%.4f' % t for t in ts)})"
    m_dev, m_host, m_ref = (sorted(ts)[REPS // 2] for ts in (t_dev, t_host, t_ref))
    say(f"{n_streams:5d} streams: step_tensor {fmt(t_dev)}, host step {fmt(t_host)}, wheel DecodeStream x {n_streams} on one thread {fmt(t_ref)}; "
        f"wheel / step_tensor {m_ref / m_dev:.2f}, wheel / host step {m_ref / m_host:.2f}")
    m_fdev, m_graph, m_fhost = (sorted(ts)[REPS // 2] for ts in (t_fdev, t_graph, t_fhost))
    say(f"{n_streams:5d} streams, fused: step_tensor {fmt(t_fdev)}, replayed graph of one step (with the ids' copy) {fmt(t_graph)}, host step {fmt(t_fhost)}; "
        f"wheel / step_tensor {m_ref / m_fdev:.2f}, wheel / graph {m_ref / m_graph:.2f}, wheel / host step {m_ref / m_fhost:.2f}; "
        f"unfused / fused step_tensor {m_dev / m_fdev:.2f}")
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
