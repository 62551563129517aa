#!/usr/bin/env python3
"""bench.py -- encode_batch throughput of the MI355X path on BASELINE.json's configs.

  python bench.py --gpus 1 --steps 20 --warmup 3                      # configs[1]: GPT-2 byte-level BPE (the headline metric)
  python bench.py --gpus 1 --steps 20 --warmup 3 --full               # the same line with every leg below (and C3 .. o200k)
  python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs bench_outputs   # + the last timed step's outputs (see below)
  python bench.py --config c3|c4|c5                                    # configs[2] / [3] / [4] on one GPU
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one pass of the whole hot path (pre-tokenize -> model -> ids CSR) over one batch that is already resident in
HBM.  Workload (default) = BASELINE.json configs[1]: GPT-2 style byte-level BPE (50,257 vocab / 50k merges, trained by the
reference's own trainer on synthetic pseudo-English), 1,000,000 synthetic ~120-byte lines per GPU per step (weak scaling:
every rank encodes its own shard; documents are independent, mod.rs:1345-1348, so the path has no exchange step and the
timed region of `value` contains no collective).  The steps ROTATE over --batches distinct batches (default 3 x 120 MB of
text, > 256 MiB with their outputs) so that neither the text nor the intermediates of one step are still in the 256 MiB
Infinity Cache when the next step reads them.

A plain run sets up, warms up, times the K steps, writes the last step's outputs if --dump-outputs DIR is given, and prints
the line: everything else below runs with --full only (tools/session.sh, the round profiles), where the objects are None
otherwise.  With --full, before anything is printed, a 2 % sample of the documents of EVERY timed batch is compared with
the CPU oracle (oracle/oracle.c): a --full line only exists for bit-exact ids.

  --dump-outputs DIR   the last timed step's token CSR (tok_offsets.npy, float64, every document) and the ids of a fixed,
                       seeded sample of its documents (ids_sample.npy, in document order; sample_docs.npy,
                       which documents; all float64, < 64 MB) -- the inputs are the same from run to run, so two builds
                       compare output for output

Rank 0 prints ONE JSON line.  Extra objects next to the contract's fields (--full):
  roofline       dominant kernel, HIP-event timed live over the same K steps; traffic from the committed PMC summary
  cpu_baseline   the reference wheel's Rayon encode_batch_fast on this box's host cores (+ 1 thread, encode_batch with
                 offsets, and the reference's 1,000-documents-per-call bench shape in `others`)
  host_boundary  the C-ABI call as SURVEY 8d times it (H2D + kernels + D2H): `value_pcie_inclusive`; from list[str] too
  out_of_distribution  the same step on text whose word types the vocabulary never saw (every word needs merges)
  word_cache     the same K steps with tkamd_word_cache on (off in `value`): warm and cold (cleared every step) figures
  single_call_multi_gpu  ONE tkamd_encode_batch on a handle over every visible GPU (sharded inside the library), per collect mode
  gather         N > 1 (or --force-gather): the same K steps ending with the RCCL collect-to-root of ids + CSR
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)


def load_config(config: str):
    from oracle import synth
    if config in ("c2", "c5"):
        return (synth.load_or_train_gpt2(), 60000,
                "BASELINE configs[1]: GPT-2 byte-level BPE 50,257 vocab / 50k merges" if config == "c2"
                else "BASELINE configs[4]: GPT-2 byte-level BPE, document lengths Zipf over 8..8192 bytes")
    if config == "o200k":
        # not a BASELINE config: the case-split member of the tiktoken Split family on the C2 corpus, with the committed
        # 3,000-entry fixture (a small vocabulary merges more words than C2's: compare with the family's other members, tools/split_family_perf.py)
        from tests.helpers import load_tokenizer_json
        return (load_tokenizer_json("split_o200k"), 60000,
                "o200k Split pattern (case-split letters, contraction suffix, [\\r\\n/]* tail) + ByteLevel + BPE, 3,000-entry vocabulary (tests/golden/split_o200k.json.gz) on the C2 corpus")
    if config == "c3":
        return synth.load_or_train_bert(), 60000, "BASELINE configs[2]: BertNormalizer + BertPreTokenizer + WordPiece 30,522 vocab"
    return synth.load_or_train_llama3(), 250000, "BASELINE configs[3]: Llama-3 style Split regex + ByteLevel + BPE 128,000 vocab (ignore_merges)"


def make_corpus(config: str, n_lines: int, text_seed: int, type_seed: int, n_types: int) -> list[str]:
    from oracle import synth
    if config == "c5":
        return synth.zipf_length_docs(n_lines * 120, text_seed=text_seed, type_seed=type_seed)
    return synth.gen_lines(n_lines, text_seed=text_seed, type_seed=type_seed, n_types=n_types)


def sample_of(lines, rank) -> tuple[list, list]:
    """The 2 % of a batch's documents the oracle gate compares: (indices, documents)."""
    idx = list(range(rank % 50, len(lines), 50))
    return idx, [lines[i] for i in idx]


def host_batch(config: str, n_lines: int, text_seed: int, type_seed: int, n_types: int, rank: int, keep_lines: bool):
    """One batch's documents, packed, with its oracle sample: (buf, off, sample, lines if keep_lines)."""
    import tokenizers_amd as ta
    lines = make_corpus(config, n_lines, text_seed, type_seed, n_types)
    buf, off = ta.pack_documents(lines)
    return buf, off, sample_of(lines, rank)[1], (lines if keep_lines else None)


def start_corpus(config: str, n_lines: int, n_batches: int, type_seed: int, n_types: int, rank: int, world: int, keep_first: bool):
    """Start making the timed batches (seeds 100 + rank + 1000 k) in worker processes -- called before torch is imported, so the
    forked workers never hold the device -- and return a function that waits for them: list of host_batch() tuples, in order.
    The same documents as making them one after the other, in a fraction of the time."""
    jobs = [(config, n_lines, 100 + rank + 1000 * k, type_seed, n_types, rank, keep_first and k == 0) for k in range(n_batches)]
    workers = max(1, min(n_batches, 8 // max(1, world)))
    if workers == 1:
        return lambda: [host_batch(*j) for j in jobs]
    import concurrent.futures
    import multiprocessing
    # (a caller that already holds the device -- a test process, say -- gets fresh interpreters instead of forks)
    holds_device = "torch" in sys.modules and sys.modules["torch"].cuda.is_initialized()
    ctx = multiprocessing.get_context("spawn" if holds_device else "fork")
    pool = concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=ctx)
    futs = [pool.submit(host_batch, *j) for j in jobs]

    def wait():
        try:
            return [f.result() for f in futs]
        finally:
            pool.shutdown()
    return wait


class Batch:
    """One batch resident in HBM + the 2 % oracle sample that vouches for it.  `packed` = a host_batch() tuple made elsewhere
    (then `lines` is not needed)."""

    def __init__(self, lines, dev, rank, keep_lines, packed=None):
        import torch
        import tokenizers_amd as ta
        if packed is None:
            buf, off = ta.pack_documents(lines)
            sample = sample_of(lines, rank)[1]
        else:
            buf, off, sample, lines = packed
        self.n_docs, self.n_bytes = len(off) - 1, int(off[-1])
        self.h_buf, self.h_off = buf, off                   # (the host-boundary leg rotates over the same batches)
        self.d_text = torch.from_numpy(buf).to(dev)
        self.d_off = torch.from_numpy(off).to(dev)
        self.sample_idx = list(range(rank % 50, self.n_docs, 50))
        self.sample = sample
        self.lines = lines if keep_lines else None
        self.n_tok = self.n_pretok = None
        self.checksum = None                                # of the result the parity gate vouched for (result_checksum)


_WEIGHTS = {}


def result_checksum(b) -> tuple:
    """Four 64-bit sums over a device result (ids and the token CSR, plain and position-weighted), computed on the device on the
    result's own stream order: equal checksums <=> (for all practical purposes) equal arrays, without a D2H of 90 MB per step."""
    import torch
    ids = b.ids_tensor().to(torch.int64)
    to = b.tok_offsets_tensor()
    n = max(ids.numel(), to.numel())
    w = _WEIGHTS.get(ids.device)
    if w is None or w.numel() < n:
        w = _WEIGHTS[ids.device] = (torch.arange(n + (n >> 2), dtype=torch.int64, device=ids.device) % 1000003) + 1
    return (int(ids.sum()), int((ids * w[:ids.numel()]).sum()), int(to.sum()), int((to * w[:to.numel()]).sum()), int(b.n_tokens))


DUMP_SEED = 20251016
DUMP_MAX_SAMPLE_TOKENS = 6_000_000      # 48 MB of float64 ids at most, next to the token CSR (8 MB per million documents)


def dump_outputs(out_dir: str, b) -> dict:
    """What a caller of the timed path receives from its last step, as float64 .npy files in out_dir: the token CSR of every
    document (tok_offsets.npy), and the ids of a fixed, seeded sample of 1 in 16 documents (sample_docs.npy: which, in order;
    ids_sample.npy: their ids, concatenated).  The sample depends on the document count alone; a sample of more than
    DUMP_MAX_SAMPLE_TOKENS ids is cut after the last whole document that fits.  Returns {name: shape}."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    ids = b.ids_tensor()
    to = b.tok_offsets_tensor().cpu().numpy()
    n_docs = to.shape[0] - 1
    docs = np.sort(np.random.default_rng(DUMP_SEED).choice(n_docs, size=max(1, n_docs // 16), replace=False)) if n_docs else np.zeros(0, np.int64)
    lens = to[docs + 1] - to[docs]
    keep = int(np.searchsorted(np.cumsum(lens), DUMP_MAX_SAMPLE_TOKENS, side="right"))
    docs, lens = docs[:keep], lens[:keep]
    # the position of every sampled token in the ids: each document's first token + 0 .. len - 1
    pos = np.repeat(to[docs] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)
    sel = ids[torch.from_numpy(pos).to(ids.device)].cpu().numpy().view(np.uint32) if pos.size else np.zeros(0, np.uint32)
    out = {"tok_offsets": to.astype(np.float64), "sample_docs": docs.astype(np.float64), "ids_sample": sel.astype(np.float64)}
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in out.items()}


def check_against_oracle(tok, oracle_obj, batch: Batch, stream) -> int:
    """ids of the batch's sample documents, HIP path vs oracle.  Returns the number of documents compared."""
    b = tok.encode_batch_device(batch.d_text.data_ptr(), batch.d_off.data_ptr(), batch.n_docs, batch.n_bytes, stream=stream).sync()
    ids = b.ids_tensor().cpu().numpy().view(np.uint32)
    to = b.tok_offsets_tensor().cpu().numpy()
    assert to[0] == 0 and to[-1] == b.n_tokens and (np.diff(to) >= 0).all(), "token CSR is not monotone"
    exp = oracle_obj.encode_batch(batch.sample)
    for k, i in enumerate(batch.sample_idx):
        g = ids[to[i]:to[i + 1]]
        e = exp.ids[exp.tok_offsets[k]:exp.tok_offsets[k + 1]]
        if len(g) != len(e) or (g != e).any():
            raise SystemExit(f"bench: PARITY FAILURE in document {i}: {batch.sample[k][:80]!r} hip={g[:12].tolist()} oracle={e[:12].tolist()}")
    batch.n_tok, batch.n_pretok = b.n_tokens, b.n_pretokens
    batch.checksum = result_checksum(b)                     # what every timed step of this batch must reproduce
    return len(batch.sample_idx)


def meta_checksum(b) -> tuple:
    """result_checksum's counterpart for the per-token (start, end) offsets and word ids of a with-offsets result."""
    import torch
    off = b.offsets_tensor().to(torch.int64)
    wid = b.word_ids_tensor().to(torch.int64)
    n = off.shape[0]
    w = _WEIGHTS.get(off.device)
    if w is None or w.numel() < n:
        w = _WEIGHTS[off.device] = (torch.arange(n + (n >> 2), dtype=torch.int64, device=off.device) % 1000003) + 1
    return result_checksum(b) + (int(off[:, 0].sum()), int((off[:, 1] * w[:n]).sum()), int((wid * w[:n]).sum()))


def check_meta_against_oracle(enc_fn, oracle_obj, batch: Batch, char: bool):
    """ids, (start, end) offsets and word ids of the batch's sample documents, HIP path vs oracle.  Returns the synced result."""
    b = enc_fn(batch).sync()
    ids = b.ids_tensor().cpu().numpy().view(np.uint32)
    offs = b.offsets_tensor().cpu().numpy().view(np.uint32)
    wid = b.word_ids_tensor().cpu().numpy().view(np.uint32)
    to = b.tok_offsets_tensor().cpu().numpy()
    exp = oracle_obj.encode_batch(batch.sample, char_offsets=char)
    for k, i in enumerate(batch.sample_idx):
        lo, hi = to[i], to[i + 1]
        elo, ehi = exp.tok_offsets[k], exp.tok_offsets[k + 1]
        if hi - lo != ehi - elo or (ids[lo:hi] != exp.ids[elo:ehi]).any():
            raise SystemExit(f"bench: PARITY FAILURE (ids, with offsets) in document {i}: {batch.sample[k][:80]!r}")
        if (offs[lo:hi] != exp.offsets[elo:ehi]).any():
            raise SystemExit(f"bench: PARITY FAILURE ({'char' if char else 'byte'} offsets) in document {i}: {batch.sample[k][:80]!r} "
                             f"hip={offs[lo:hi][:8].tolist()} oracle={exp.offsets[elo:ehi][:8].tolist()}")
        if (wid[lo:hi] != exp.words[elo:ehi]).any():
            raise SystemExit(f"bench: PARITY FAILURE (word ids) in document {i}: {batch.sample[k][:80]!r}")
    return b


OFFSET_KERNELS = ("emit_pretok", "leadmask_scan", "token_meta")


def offsets_leg(tok, oracle_obj, batches, stream, steps: int, mode: str, b_alg_ids: float, config: str) -> dict:
    """The function BASELINE's metric NAMES: Rust `encode_batch` returns byte offsets + word ids (tokenizer/mod.rs:1337-1356), Python's
    `encode_batch` char offsets + word ids (mod.rs:1360-1379); `value` above is `encode_batch_fast` (ids only, mod.rs:1382-1401).  The same K
    steps over the same rotating HBM-resident batches with TKAMD_OFFSETS_BYTE|CHAR + TKAMD_WANT_WORD_IDS: a 2 % oracle gate on ids, offsets
    and word ids of every batch, wall clock between device synchronisations, checksums of the timed outputs, per-kernel HIP-event times,
    and a roofline on SURVEY 8d's bytes (B_alg + 8 T offsets + 4 T word ids)."""
    import torch
    n_batches = len(batches)
    char = mode == "char"

    def enc_b(b):
        return tok.encode_batch_device(b.d_text.data_ptr(), b.d_off.data_ptr(), b.n_docs, b.n_bytes, offsets=mode, word_ids=True, stream=stream)

    def enc(i):
        return enc_b(batches[i % n_batches])
    sums = [meta_checksum(check_meta_against_oracle(enc_b, oracle_obj, b, char)) for b in batches]
    n_checked = sum(len(b.sample_idx) for b in batches)
    for i in range(3 * n_batches):
        enc(i)
    torch.cuda.synchronize()
    blocks = []
    last = None
    for _ in range(4):
        t_s = time.perf_counter()
        for i in range(steps):
            last = enc(i)
        last.sync()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t_s) / steps)
    if meta_checksum(last) != sums[(steps - 1) % n_batches]:
        raise SystemExit(f"bench: the last timed with-offsets step ({mode}) differs from the gated result of its batch")
    for i in range(n_batches):
        if meta_checksum(enc(i).sync()) != sums[i]:
            raise SystemExit(f"bench: a re-run with-offsets step ({mode}) differs from the gated result of its batch")
    tok.profile(True)
    for i in range(steps):
        enc(i)
    enc(steps).sync()
    tok.profile(False)
    stages = {k: v[0] / max(1, v[1]) for k, v in tok.profile_read().items()}
    n_bytes = sum(batches[i % n_batches].n_bytes for i in range(steps)) / steps
    n_tok = sum(batches[i % n_batches].n_tok for i in range(steps)) / steps
    b_alg = b_alg_ids + 12.0 * n_tok
    first, srt = blocks[0], sorted(blocks[1:])
    med = srt[len(srt) // 2]
    dom = max(stages, key=stages.get)
    ach = b_alg / (stages[dom] * 1e-3) / 1e9
    okern = {}
    for k in OFFSET_KERNELS:
        if k in stages:
            tr, src = pmc_traffic(k, config)
            # what the offsets kernels must move between them: 8 T offsets + 4 T word ids out; their inputs (masks, rows,
            # pre-token starts) are intermediates of the path
            okern[k] = {"ms": round(stages[k], 4), "traffic": tr, "traffic_source": src}
    t_off = sum(stages.get(k, 0.0) for k in OFFSET_KERNELS)
    return {"offsets": mode, "word_ids": True,
            "reference_function": "TokenizerImpl::encode_batch_char_offsets (tokenizer/mod.rs:1360-1379; Python's encode_batch)" if char
                                  else "TokenizerImpl::encode_batch (tokenizer/mod.rs:1337-1356)",
            "value": round(n_bytes / first / 1e9, 3), "unit": "GB/s", "ms_per_step": round(first * 1e3, 4),
            "value_median": round(n_bytes / med / 1e9, 3), "ms_per_step_blocks": [round(x * 1e3, 4) for x in blocks],
            "mtokens_per_s": round(n_tok / first / 1e6, 2), "steps": steps,
            "parity": {"checked_documents": n_checked, "against": "oracle/oracle.c", "of": "every timed batch (2 % sample): ids, offsets and word ids bit-exact",
                       "timed_outputs": "checksums of ids, token CSR, offsets and word ids of the last timed step and of one re-run per batch equal the gated results'"},
            "roofline": {"bound": "hbm", "kernel": dom, "kernel_ms": round(stages[dom], 4), "achieved": round(ach, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBPS, 5), "algorithmic_bytes_per_launch": int(b_alg),
                         "whole_path_frac": round(b_alg / first / 1e9 / HBM_PEAK_GBPS, 5),
                         "offsets_kernels": okern, "offsets_kernels_ms": round(t_off, 4),
                         "offsets_kernels_algorithmic_bytes": int(12.0 * n_tok),
                         "offsets_kernels_achieved": round(12.0 * n_tok / (t_off * 1e-3) / 1e9, 2) if t_off else None,
                         "all_kernels_ms": {k: round(v, 4) for k, v in stages.items()}, "sum_kernels_ms": round(sum(stages.values()), 4)}}


def timed_steps(step_fn, steps: int, warmup: int, fence, reduce_max, finish_last=None) -> float:
    """The contract's timed region: W untimed warm-up steps, then EXACTLY K steps between two fences (barrier + device
    synchronisation on both sides), and the MAX over ranks of the wall time.  `fence()` / `reduce_max(seconds) -> seconds` carry
    the process group (no-ops for one rank); `finish_last(x)` waits for what the last step returned.  Kept free of CUDA so that
    tests/test_parallel.py runs this very function over gloo with a stand-in step."""
    for i in range(warmup):
        step_fn(i)
    fence()
    t_start = time.perf_counter()
    last = None
    for i in range(steps):
        last = step_fn(i)
    if finish_last is not None and last is not None:
        finish_last(last)
    fence()
    return reduce_max(time.perf_counter() - t_start), last


def run_guarded(fn, seconds: float, on_timeout):
    """fn() under a watchdog THREAD (not SIGALRM: a rank stuck inside a collective sits in C++ with the GIL released, where a Python
    signal handler never gets to run; a thread does).  on_timeout() runs on the watchdog thread and is expected not to return
    (bench.py prints what it has and os._exit()s, on every rank, so that a hang ends the whole job)."""
    import threading
    wd = threading.Timer(seconds, on_timeout)
    wd.daemon = True
    wd.start()
    try:
        return fn()
    finally:
        wd.cancel()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lines", type=int, default=1_000_000, help="documents per GPU per step")
    ap.add_argument("--batches", type=int, default=3, help="distinct batches the steps rotate over (working set > Infinity Cache)")
    ap.add_argument("--gather", action="store_true", help="(kept for old command lines: the gather leg always runs when N > 1)")
    ap.add_argument("--no-gather", action="store_true", help="skip the gather leg")
    ap.add_argument("--force-gather", action="store_true", help="run the gather leg even with one rank (self-test of the RCCL path)")
    ap.add_argument("--repeat-blocks", type=int, default=5, help="further blocks of K steps timed like the contract's one (min / median / max in `repeat`)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ood", action="store_true", help="skip the out-of-distribution leg")
    ap.add_argument("--no-host", action="store_true", help="skip the host-boundary leg")
    ap.add_argument("--no-word-cache", action="store_true", help="skip the word-cache leg")
    ap.add_argument("--no-offsets", action="store_true", help="skip the with-offsets legs (encode_batch with byte / char offsets + word ids)")
    ap.add_argument("--no-single-call", action="store_true", help="skip the single-call multi-GPU leg")
    ap.add_argument("--single-call-gpus", type=int, default=0, help="devices of the single-call leg (0 = every visible GPU)")
    ap.add_argument("--cpu-lines", type=int, default=0, help="lines for the CPU baseline sample (0 = auto)")
    ap.add_argument("--cpu-brief", action="store_true", help="CPU baseline: the all-cores encode_batch_fast and encode_batch figures only")
    ap.add_argument("--type-seed", type=int, default=0, help="word-type seed of the ENCODED text (0 = in-distribution)")
    ap.add_argument("--also", default="c3,c4,c5,o200k", help="(N = 1, --config c2 only) further BASELINE configs timed by child runs of this script after the "
                                                     "headline measurement and attached as `other_configs`; 'none' = skip")
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "c4", "c5", "o200k"],
                    help="BASELINE.json config: c2 GPT-2 BPE (the headline metric, default), c3 BERT WordPiece, "
                         "c4 Llama-3 style BPE 128k, c5 GPT-2 BPE on Zipf-length documents")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure as well: the oracle parity gate and the check of the timed outputs, the repeat "
                         "blocks, the roofline, with-offsets, word-cache, out-of-distribution, host-boundary, single-call and CPU-baseline legs, "
                         "the other configs (--also) and, at N > 1, the gather leg; the --no-* options trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR as .npy (float64): tok_offsets, sample_docs, ids_sample")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world == 1 and args.gpus > 1:
        raise SystemExit("launch multi-GPU runs with torch.distributed.run (one process per GPU)")
    t0 = time.time()
    tok_json, n_types, workload = load_config(args.config)
    n_batches = max(1, args.batches)
    # (the host leg, the single-call leg and the CPU baseline read the first batch's documents as strings)
    corpus = start_corpus(args.config, args.lines, n_batches, args.type_seed, n_types, rank, world, keep_first=args.full)

    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_gather
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)

    from oracle import oracle as orc      # the checker (and the cpu_baseline fallback): never the thing measured
    from oracle import synth
    import tokenizers_amd as ta
    from tokenizers_amd.parallel import gather_to_root

    tok = ta.Tokenizer.from_str(tok_json, device=local_rank)
    oracle_obj = orc.Oracle(tok_json) if args.full else None
    log(f"[bench] tokenizer ready in {time.time() - t0:.1f}s  sha256={synth.sha256(tok_json)[:12]} info={tok.info}")

    t0 = time.time()
    batches = [Batch(None, dev, rank, keep_lines=(k == 0), packed=p) for k, p in enumerate(corpus())]
    log(f"[bench] corpus: {n_batches} batches of {batches[0].n_docs} docs / {batches[0].n_bytes / 1e6:.1f} MB in {time.time() - t0:.1f}s more")
    stream = torch.cuda.current_stream().cuda_stream

    # ---- parity gate (--full): a 2 % sample of every timed batch against the oracle, before any timing counts ----
    n_checked = None
    if args.full:
        t0 = time.time()
        n_checked = sum(check_against_oracle(tok, oracle_obj, b, stream) for b in batches)
        log(f"[bench] parity: {n_checked} sampled documents of the timed batches equal the oracle ({time.time() - t0:.1f}s)")

    def encode(i):
        b = batches[i % n_batches]
        return tok.encode_batch_device(b.d_text.data_ptr(), b.d_off.data_ptr(), b.n_docs, b.n_bytes, stream=stream)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def reduce_max(seconds):
        el = torch.tensor([seconds], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        return float(el.item())

    def timed(step_fn):
        """W untimed + exactly K timed steps, barrier + synchronize on both sides, MAX over ranks."""
        el, last = timed_steps(step_fn, args.steps, args.warmup, fence, reduce_max, finish_last=lambda b: b.sync())
        state["last"] = last
        return el

    state = {}
    # (un-timed, in front of the contract's W warm-up steps: twenty full rotations over the batches -- some thirty milliseconds of the
    # same work -- so that clocks, the workspaces and the handle's claims statistics are where the repeat blocks find them: round 5's
    # first block ran 2.5 % behind the later ones, with three rotations round 6's still 0.6 %)
    # (the first rotation also learns each batch's token and pre-token counts where no parity gate has: the line's token rate)
    for i in range(20 * n_batches):
        r = encode(i)
        if i < n_batches and batches[i].n_tok is None:
            r.sync()
            batches[i].n_tok, batches[i].n_pretok = r.n_tokens, r.n_pretokens
    torch.cuda.synchronize()
    elapsed = timed(encode)
    if args.dump_outputs and rank == 0:
        t0 = time.time()
        shapes = dump_outputs(args.dump_outputs, state["last"])
        log(f"[bench] outputs of the last timed step in {args.dump_outputs}: {shapes} ({time.time() - t0:.1f}s)")
    # ---- (--full) the same measurement again, `repeat_blocks` times: K steps between the same fences, max over ranks.  The contract's
    # block is 20 steps of about half a millisecond -- eleven milliseconds; min / median / max over five more say how much of a 2-3 %
    # difference between two builds is the box (every rank takes part: reduce_max is a collective). ----
    rep_ms = []
    for _ in range(max(0, args.repeat_blocks) if args.full else 0):
        el, _ = timed_steps(encode, args.steps, 0, fence, reduce_max, finish_last=lambda b: b.sync())
        rep_ms.append(el / args.steps * 1e3)
    # ---- the outputs of the timed region: the LAST timed step's ids + token CSR (still in the workspace) must be the result the
    # parity gate vouched for, and so must every step of one more pass over the same K-step sequence (un-timed: the checksum runs
    # on the stream behind each encode) -- with in-batch claims a repeat's result depends on a row another workgroup publishes, so
    # "the gate passed once" is not the same statement as "the timed steps produced these ids". ----
    n_verified = 0
    if args.full:
        last_b = batches[(args.steps - 1) % n_batches]
        if result_checksum(state["last"]) != last_b.checksum:
            raise SystemExit("bench: the last TIMED step's ids / token CSR differ from the result the parity gate checked for that batch")
        for i in range(args.steps):
            if result_checksum(encode(i).sync()) != batches[i % n_batches].checksum:
                raise SystemExit(f"bench: step {i} of the verification pass produced ids / token CSR that differ from the parity gate's")
            n_verified += 1
        log(f"[bench] timed outputs: last timed step + {n_verified} re-run steps reproduce the gate's checksums")
    # units all ranks processed in the K timed steps
    mine = np.zeros(4, dtype=np.float64)
    for i in range(args.steps):
        b = batches[i % n_batches]
        mine += [b.n_bytes, b.n_tok, b.n_docs, b.n_pretok]
    tot = torch.tensor(mine, dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    tot_bytes, tot_tok, tot_docs, tot_pretok = (float(x) for x in tot.tolist())
    ms_per_step = elapsed / args.steps * 1e3
    gbps = tot_bytes / elapsed / 1e9
    repeat = None
    if rep_ms:
        srt = sorted(rep_ms)
        med = srt[len(srt) // 2] if len(srt) % 2 else 0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2])
        repeat = {"blocks": len(rep_ms), "steps_per_block": args.steps, "ms_per_step": [round(x, 4) for x in rep_ms],
                  "ms_per_step_min": round(srt[0], 4), "ms_per_step_median": round(med, 4), "ms_per_step_max": round(srt[-1], 4),
                  "value_median": round(tot_bytes / args.steps / (med * 1e-3) / 1e9, 3), "unit": "GB/s",
                  "note": "further blocks of K steps, each timed exactly like the contract's block (`ms_per_step` / `value` above are that first block alone)"}
    mtoks = tot_tok / elapsed / 1e6

    def finish(gather_obj):
        if rank != 0 or state.get("done"):
            return
        state["done"] = True
        out = dict(state["out"])
        out["gather"] = gather_obj
        print(json.dumps(out), flush=True)

    # ---- roofline leg: per-kernel HIP-event times over the same K steps (rank 0) ----
    roofline = None
    if rank == 0 and args.full:
        tok.profile(True)
        for i in range(args.steps):
            encode(i)
        encode(args.steps).sync()
        tok.profile(False)
        stages = {k: v[0] / max(1, v[1]) for k, v in tok.profile_read().items()}   # ms per launch
        dom = max(stages, key=stages.get)
        # algorithmic bytes of the whole path per launch: text in + doc CSR in + ids out + token CSR out
        b_alg = (mine[0] + 8 * (mine[2] + args.steps) + 4 * mine[1] + 8 * (mine[2] + args.steps)) / args.steps
        achieved = b_alg / (stages[dom] * 1e-3) / 1e9
        traffic, traffic_source = pmc_traffic(dom, args.config)
        traffic_stale = bool(traffic_source and traffic_source.get("traffic_stale"))
        roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": traffic, "traffic_stale": traffic_stale,
                    # (traffic is NOT re-measured in this run -- PMC passes need rocprofv3 around the process: it is the committed summary's
                    # figure for this kernel, per launch; the file and the commit it was taken on)
                    "traffic_source": traffic_source,
                    "algorithmic_bytes_per_launch": int(b_alg), "kernel_ms": round(stages[dom], 4),
                    "whole_path_frac": round(b_alg / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBPS, 5),
                    "all_kernels_ms": {k: round(v, 4) for k, v in stages.items()},
                    "sum_kernels_ms": round(sum(stages.values()), 4), "merge_queue_sizes": tok.queue_sizes()}
        if traffic:
            # what the fabric actually carried while the kernel ran (the committed PMC summary's bytes per launch over THIS run's kernel
            # time): the kernel's distance from the bandwidth roofline on the bytes it fetches, next to `frac` on the bytes it needs
            roofline["traffic_gbps"] = round(traffic / (stages[dom] * 1e-3) / 1e9, 1)
            roofline["traffic_frac"] = round(traffic / (stages[dom] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
            roofline["traffic_over_algorithmic"] = round(traffic / b_alg, 2)
        # SURVEY 8d's secondary model for the merge kernels: (k - 1) + 2 m merge-table probes for a word of k symbols and m merges,
        # counted by the kernels themselves during this (profiling) pass for the batch that ran last
        qs = roofline["merge_queue_sizes"]
        mk = [k for k in stages if k.startswith("bpe_merge_lds")]
        if qs.get("merge_probes") and mk:
            t_merge = sum(stages[k] for k in mk) * 1e-3
            roofline["merge_probes"] = {"per_batch": int(qs["merge_probes"]), "words": int(qs["merge16"] + qs["merge32"]),
                                        "probes_per_s": round(qs["merge_probes"] / t_merge / 1e9, 3), "unit": "G probes/s",
                                        "kernels_ms": round(t_merge * 1e3, 4), "bytes_per_probe": 16,
                                        "model": "(k - 1) + 2 m per queued word of k symbols and m merges; the in-batch claims leave the distinct words only"}

    # ---- with-offsets legs (rank 0, N=1): the functions the metric names -- Rust encode_batch (byte offsets + word ids) and Python's
    # encode_batch (char offsets + word ids); `value` above is encode_batch_fast ----
    with_off = None
    if rank == 0 and world == 1 and args.full and not args.no_offsets:
        with_off = {}
        for mode in ("byte", "char"):
            t0 = time.time()
            try:
                with_off[mode] = offsets_leg(tok, oracle_obj, batches, stream, args.steps, mode, b_alg, args.config)
                with_off[mode]["ratio_to_value"] = round(with_off[mode]["value"] / gbps, 3)
            except SystemExit:
                raise
            except Exception as ex:     # never lose the bench line to an auxiliary leg
                with_off[mode] = {"error": repr(ex)[:300]}
            log(f"[bench] with-offsets leg ({mode}) in {time.time() - t0:.1f}s: {with_off[mode].get('value', with_off[mode].get('error'))}")

    # ---- word-cache leg (rank 0, N=1): the device-side counterpart of the reference's per-thread word cache
    # (models/bpe/model.rs:573-586).  NOT `value`: the steps revisit the same three batches, so a warm cache has seen every word of
    # them -- the upper end of what a long-running service sees; the cold figure (cache cleared before every step: every queued word
    # is merged AND inserted) is the lower end. ----
    wcache = None
    if rank == 0 and world == 1 and args.full and not args.no_word_cache:
        tok.word_cache(True, clear=True)
        for i in range(n_batches):
            encode(i)
        encode(0).sync()
        sizes_warm = tok.queue_sizes()
        torch.cuda.synchronize()
        t_s = time.perf_counter()
        for i in range(args.steps):
            last = encode(i)
        last.sync()
        torch.cuda.synchronize()
        dt_warm = (time.perf_counter() - t_s) / args.steps
        tok.profile(True)
        for i in range(6):
            encode(i)
        encode(0).sync()
        tok.profile(False)
        wst = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
        n_cold = min(args.steps, 6)
        torch.cuda.synchronize()
        t_s = time.perf_counter()
        for i in range(n_cold):
            tok.word_cache(True, clear=True)
            last = encode(i)
        last.sync()
        torch.cuda.synchronize()
        dt_cold = (time.perf_counter() - t_s) / n_cold
        for b in batches:                                    # parity with a warm cache: the same oracle sample as the gate above
            check_against_oracle(tok, oracle_obj, b, stream)
        tok.word_cache(False, clear=True)
        bytes_per_step = tot_bytes / args.steps
        wcache = {"value_warm": round(bytes_per_step / dt_warm / 1e9, 3), "ms_per_step_warm": round(dt_warm * 1e3, 4),
                  "value_cold": round(bytes_per_step / dt_cold / 1e9, 3), "ms_per_step_cold": round(dt_cold * 1e3, 4), "unit": "GB/s",
                  "merge_queue_sizes_warm": sizes_warm, "all_kernels_ms_warm": {k: v for k, v in wst.items() if v >= 0.004},
                  "note": "tkamd_word_cache on (off by default and in `value`): warm = the rotating batches after one pass over them "
                          "(every word of them cached), cold = cache cleared before every step; oracle sample re-checked with the cache warm"}

    # ---- out-of-distribution leg (rank 0, N=1): word types the vocabulary never saw -> every word runs the merge loop ----
    ood = None
    if rank == 0 and world == 1 and args.full and not args.no_ood and args.type_seed == 0:
        t0 = time.time()
        ob = Batch(make_corpus(args.config, args.lines, 100, 1, n_types), dev, rank, keep_lines=False)
        check_against_oracle(tok, oracle_obj, ob, stream)

        def enc_ood(i):
            return tok.encode_batch_device(ob.d_text.data_ptr(), ob.d_off.data_ptr(), ob.n_docs, ob.n_bytes, stream=stream)
        for i in range(2):
            enc_ood(i)
        torch.cuda.synchronize()
        t_s = time.perf_counter()
        for i in range(10):
            last = enc_ood(i)
        last.sync()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t_s) / 10
        tok.profile(True)
        for i in range(5):
            enc_ood(i)
        enc_ood(0).sync()
        tok.profile(False)
        ost = {k: round(v[0] / max(1, v[1]), 4) for k, v in tok.profile_read().items()}
        ood = {"type_seed": 1, "value": round(ob.n_bytes / dt / 1e9, 3), "unit": "GB/s", "ms_per_step": round(dt * 1e3, 4),
               "tokens": int(ob.n_tok), "pretokens": int(ob.n_pretok), "merge_queue_sizes": tok.queue_sizes(),
               "all_kernels_ms": {k: v for k, v in ost.items() if v >= 0.004},
               "note": "one 1M-line batch (no rotation), 2 % of it checked against the oracle; same vocabulary, unseen word types"}
        del ob
        log(f"[bench] out-of-distribution leg in {time.time() - t0:.1f}s")

    # ---- host-boundary leg (rank 0, N=1): the C-ABI call of SURVEY 8d = H2D + kernels + D2H (PCIe inclusive) ----
    host = None
    if rank == 0 and world == 1 and args.full and not args.no_host:
        lines = batches[0].lines
        t0 = time.perf_counter()
        hb, ho = ta.pack_documents(lines)
        t_pack = time.perf_counter() - t0
        # measured like `value`: W warm-up calls, then K calls rotating over the same distinct batches, wall clock over all of them
        n_host = max(3, min(args.steps, 12))
        for i in range(min(args.warmup, n_batches) or 1):
            tok.encode_packed(batches[i % n_batches].h_buf, batches[i % n_batches].h_off)      # warm-up (staging buffers, pinned blocks)
        best = float("inf")
        host_bytes = 0
        t_all = time.perf_counter()
        for i in range(n_host):
            hbk = batches[i % n_batches]
            t0 = time.perf_counter()
            res = tok.encode_packed(hbk.h_buf, hbk.h_off)
            best = min(best, time.perf_counter() - t0)
            host_bytes += hbk.n_bytes
            assert res.n_tokens == hbk.n_tok
        t_all = time.perf_counter() - t_all
        # the same calls with the packed documents in page-locked memory from tkamd_pinned_alloc (a binding packs the documents into
        # ONE buffer for this ABI anyway: packing into a pinned block costs it nothing extra, and the H2D copies run as plain DMA)
        pinned = [(ta.pinned_copy(bk.h_buf), ta.pinned_copy(bk.h_off)) for bk in batches]
        for i in range(min(args.warmup, n_batches) or 1):
            tok.encode_packed(*pinned[i % n_batches])
        best_p = float("inf")
        t_pin = time.perf_counter()
        for i in range(n_host):
            t0 = time.perf_counter()
            res = tok.encode_packed(*pinned[i % n_batches])
            best_p = min(best_p, time.perf_counter() - t0)
            assert res.n_tokens == batches[i % n_batches].n_tok
        t_pin = time.perf_counter() - t_pin
        same = bool((res.ids == tok.encode_packed(batches[(n_host - 1) % n_batches].h_buf, batches[(n_host - 1) % n_batches].h_off).ids).all())
        del pinned
        res = tok.encode_packed(hb, ho)
        host = {"pack_list_of_str_ms": round(t_pack * 1e3, 2), "encode_packed_ms": round(t_pin / n_host * 1e3, 2),
                "encode_packed_best_ms": round(best_p * 1e3, 2), "calls": n_host,
                "gbps_pcie_inclusive": round(host_bytes / t_pin / 1e9, 3),
                "encode_packed_pageable_ms": round(t_all / n_host * 1e3, 2), "encode_packed_pageable_best_ms": round(best * 1e3, 2),
                "gbps_pcie_inclusive_pageable": round(host_bytes / t_all / 1e9, 3),
                "pinned_equals_pageable": same,
                "gbps_from_list_of_str": round(batches[0].n_bytes / (t_pin / n_host + t_pack) / 1e9, 3),
                "note": "tkamd_encode_batch wall clock: H2D of text + CSR, kernels, D2H of ids + CSR into pinned host memory; mean over "
                        "`calls` back-to-back calls rotating over the timed batches (best single call next to it).  Caller buffers from "
                        "tkamd_pinned_alloc; `_pageable`: ordinary (numpy) memory"}
        assert res.n_tokens == batches[0].n_tok
        try:        # the same from a Python list[str] through the tokenizer's reusable staging (what a caller of encode_batch_fast feels)
            tok.encode_batch_fast(lines, add_special_tokens=False)
            best2 = float("inf")
            for _ in range(3):
                t0 = time.perf_counter()
                r2 = tok.encode_batch_fast(lines, add_special_tokens=False)
                best2 = min(best2, time.perf_counter() - t0)
            host["encode_batch_fast_list_of_str_ms"] = round(best2 * 1e3, 2)
            host["gbps_encode_batch_fast_list_of_str"] = round(batches[0].n_bytes / best2 / 1e9, 3)
            if r2.n_tokens != batches[0].n_tok:
                host["encode_batch_fast_list_of_str_error"] = "token count differs"
        except Exception as ex:     # never lose the bench line to the auxiliary leg
            host["encode_batch_fast_list_of_str_error"] = repr(ex)

    # ---- single-call multi-GPU leg (rank 0, one process): ONE tkamd_encode_batch on a handle made over a device list; the library
    # shards the documents by bytes, one host thread + stream per device, and the shards' results meet per collect mode
    # (include/tokenizers_amd.h "one call, every GPU"; the reference: one encode_batch call uses the whole Rayon pool,
    # tokenizer/mod.rs:1345-1348).  PCIe inclusive by construction (host buffers in, host buffers out).  With one visible GPU the list
    # names it twice: the code path runs, the figure says nothing about scaling. ----
    single_call = None
    if rank == 0 and world == 1 and args.full and not args.no_host and not args.no_single_call:
        try:
            if torch.cuda.device_count() < 2:
                single_call = single_call_leg(ta, tok_json, batches[0].lines, 1, args.single_call_gpus)
            else:
                # several GPUs visible: this is the first time the sharded path meets real peers -- in a child process under a
                # timeout, one JSON line per collect mode, so that a hang costs the leg (what it printed so far is kept), not the line
                single_call = single_call_child(args.config, batches[0].n_docs, args.type_seed, args.single_call_gpus)
        except Exception as ex:     # never lose the bench line to an auxiliary leg
            single_call = {"error": repr(ex)[:300]}

    # ---- CPU baseline leg (rank 0, N=1 only): the reference's Rayon encode_batch on the host cores ----
    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(tok_json, batches[0].lines, args.cpu_lines, args.config, brief=args.cpu_brief)

    # ---- the other BASELINE configs on this GPU (rank 0, N=1, headline config only): the same script, same flags, as child processes
    # one after the other -- so that C3 / C4 are driver-timed numbers too, not only builder-run ones ----
    others_cfg = None
    also = [c.strip() for c in args.also.split(",") if c.strip() in ("c3", "c4", "c5", "o200k")]
    if rank == 0 and world == 1 and args.full and args.config == "c2" and also:
        others_cfg = {}
        for cfg in also:
            t0 = time.time()
            others_cfg[cfg] = other_config_leg(cfg, args.steps, args.warmup, args.lines, n_batches)
            log(f"[bench] {cfg} leg in {time.time() - t0:.1f}s: {others_cfg[cfg].get('value', others_cfg[cfg].get('error'))}")

    if rank == 0:
        b0 = batches[0]
        state["out"] = {
            "metric": ("GB input text/sec (whole node), GPT-2 BPE encode_batch" if args.config in ("c2", "c5")
                       else f"GB input text/sec (whole node), encode_batch [{args.config}]"),
            "value": round(gbps, 3), "unit": "GB/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8->u32", "data": "synthetic",
            "mtokens_per_s": round(mtoks, 2), "repeat": repeat,
            "value_definition": "input text bytes of all ranks / max-over-ranks wall time of the K steps with inputs already resident in HBM "
                                "when the timed region starts and outputs left in HBM -- the task statement pins `value` to exactly that ("
                                "'whole-job throughput with inputs already resident in HBM ...; the PCIe-inclusive rate ... is never value'). "
                                "SURVEY 8d's wall clock of the C-ABI host call (H2D + kernels + D2H) is value_pcie_inclusive, measured the same "
                                "way (warm-up, then back-to-back calls rotating over the same batches); at N > 1 the 8d whole-node figure "
                                "including the RCCL collect is gather.value",
            "value_pcie_inclusive": host["gbps_pcie_inclusive"] if host else None,
            "value_from_python_list_of_str": host.get("gbps_encode_batch_fast_list_of_str") if host else None,
            "value_with_offsets": (with_off or {}).get("byte", {}).get("value"),
            "value_with_char_offsets": (with_off or {}).get("char", {}).get("value"),
            "value_out_of_distribution": ood["value"] if ood else None,
            "value_with_word_cache": wcache["value_warm"] if wcache else None,
            "parity": {"checked_documents": int(n_checked), "against": "oracle/oracle.c", "of": "every timed batch (2 % sample), ids bit-exact",
                       "timed_outputs": f"checksums of ids + token CSR of the last timed step and of {n_verified} re-run steps equal the gated results'"}
                      if args.full else None,
            "config": {"workload": f"{workload}, {b0.n_docs} synthetic documents ({b0.n_bytes / 1e6:.0f} MB) per GPU per step, "
                                   f"{n_batches} distinct batches rotated, ids-only (encode_batch_fast), inputs resident in HBM",
                       "docs_per_gpu": b0.n_docs, "bytes_per_gpu": b0.n_bytes, "tokens_per_gpu": int(b0.n_tok),
                       "pretokens_per_gpu": int(b0.n_pretok), "batches": n_batches, "type_seed": args.type_seed,
                       "tokenizer_sha256": synth.sha256(tok_json)[:16],
                       "parallelism": f"dp{world} (documents sharded by rank)"},
            "roofline": roofline, "with_offsets": with_off, "cpu_baseline": cpu, "host_boundary": host, "single_call_multi_gpu": single_call,
            "out_of_distribution": ood, "word_cache": wcache, "other_configs": others_cfg,
        }
    # ---- gather leg: the same K steps, each ending with the collect-to-root of the final buffers over RCCL ----
    gather_obj = None
    if (args.force_gather or (world > 1 and args.full)) and not args.no_gather:
        # A collective that never completes must not cost the bench line.  A watchdog THREAD, not SIGALRM: a rank stuck inside a RCCL
        # wait sits in C++ with the GIL released, where a Python signal handler never gets to run; a thread does.  Every rank has
        # one (rank 0 prints the line first), so a hang ends the whole job instead of leaving torchrun waiting on the others.
        def on_timeout():
            finish({"error": "the gather leg did not finish within 180 s"})
            os._exit(0)

        def step_gather(i):
            b = encode(i)
            gather_to_root(b.ids_tensor_unsynced(), b.tok_offsets_tensor(), dev, n_tokens_dev=b.n_tokens_tensor())
            return b
        try:
            el_g = run_guarded(lambda: timed(step_gather), 180.0, on_timeout)
            gather_obj = {"ms_per_step": round(el_g / args.steps * 1e3, 4), "value": round(tot_bytes / el_g / 1e9, 3), "unit": "GB/s",
                          "what": "the same K steps, each followed by gather_to_root (one all_gather of sizes + one point-to-point message per "
                                  "peer for ids and per-document counts) over RCCL; the root's copy of its own shard included"}
        except Exception as ex:
            gather_obj = {"error": repr(ex)}
    finish(gather_obj)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def other_config_leg(cfg: str, steps: int, warmup: int, n_lines: int, n_batches: int, timeout_s: int = 420) -> dict:
    """`python bench.py --config cfg --full` (kernel pipeline + parity gate + roofline leg only) as a child process; the fields of its line
    that matter, or an error -- never an exception (the headline line must not be lost to an auxiliary leg)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--full", "--steps", str(steps), "--warmup", str(warmup), "--lines", str(n_lines),
           "--batches", str(n_batches), "--cpu-lines", str(min(n_lines, 250_000)), "--cpu-brief", "--no-ood", "--no-host", "--no-word-cache",
           "--no-single-call", "--also", "none"] + (["--no-offsets"] if cfg == "c5" else [])
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout_s)
        line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
        if line is None:
            return {"error": f"no line (exit {r.returncode}): {r.stderr[-300:]}"}
        j = json.loads(line)
        rf = j.get("roofline") or {}
        return {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "mtokens_per_s": j.get("mtokens_per_s"),
                "steps": j["steps"], "workload": j["config"]["workload"], "parity": j.get("parity"),
                "roofline": {k: rf.get(k) for k in ("kernel", "kernel_ms", "achieved", "frac", "whole_path_frac", "traffic", "traffic_source", "all_kernels_ms")},
                "repeat": j.get("repeat"), "value_with_offsets": j.get("value_with_offsets"), "value_with_char_offsets": j.get("value_with_char_offsets"),
                "with_offsets": j.get("with_offsets"), "cpu_baseline": j.get("cpu_baseline")}
    except subprocess.TimeoutExpired:
        return {"error": f"child killed after {timeout_s} s"}
    except Exception as ex:
        return {"error": repr(ex)[:300]}


def single_call_items(ta, tok_json: str, lines: list, n_visible: int, want: int):
    """One host-entry call over a device list, per collect mode: best of 3 wall clocks of `encode_packed` on n_dev x the batch.
    Yields (key, value) pairs as they are measured."""
    n_dev = want or n_visible
    emulated = n_visible < 2
    devices = [0, 0] if emulated else list(range(min(n_dev, n_visible)))
    hb0, ho0 = ta.pack_documents(lines)
    n_docs = len(lines)
    k = len(devices)
    nb0 = int(ho0[-1])
    hb = np.empty(nb0 * k + 64, dtype=np.uint8)
    ho = np.empty(n_docs * k + 1, dtype=np.int64)
    for r in range(k):                                       # the batch n_dev times over: every device gets the batch's work
        hb[r * nb0:(r + 1) * nb0] = hb0[:nb0]
        ho[r * n_docs:(r + 1) * n_docs + 1] = ho0 + r * nb0
    yield "devices", devices
    yield "emulated_on_one_gpu", emulated
    yield "bytes", nb0 * k
    yield "docs", n_docs * k
    yield "unit", "GB/s"
    yield "what", "wall clock of ONE tkamd_encode_batch (pageable host text in, pinned ids + CSR out) on a multi-device handle, best of 3"
    one = ta.Tokenizer.from_str(tok_json, device=devices[0])
    one.encode_packed(hb, ho)
    best, ref = float("inf"), None
    for _ in range(3):
        t0 = time.perf_counter()
        ref = one.encode_packed(hb, ho)
        best = min(best, time.perf_counter() - t0)
    yield "one_device", {"ms": round(best * 1e3, 2), "value": round(nb0 * k / best / 1e9, 3)}
    for mode in ("host", "p2p") + (() if emulated else ("rccl",)):
        try:
            many = ta.Tokenizer.from_str(tok_json, device=devices, collect=mode)
            many.encode_packed(hb, ho)                       # warm-up: workspaces, pinned blocks, (rccl) the communicators
            best, res = float("inf"), None
            for _ in range(3):
                t0 = time.perf_counter()
                res = many.encode_packed(hb, ho)
                best = min(best, time.perf_counter() - t0)
            same = res.n_tokens == ref.n_tokens and bool((res.ids == ref.ids).all()) and bool((res.tok_offsets == ref.tok_offsets).all())
            st = many.shard_stats()
            busy = [ms for _, _, ms in st]
            yield mode, {"ms": round(best * 1e3, 2), "value": round(nb0 * k / best / 1e9, 3), "equals_one_device": same,
                         "busy_ms_max_over_mean": round(max(busy) / (sum(busy) / len(busy)), 3) if busy else None}
            del many
        except Exception as ex:
            yield mode, {"error": repr(ex)[:300]}


def single_call_leg(ta, tok_json: str, lines: list, n_visible: int, want: int) -> dict:
    return dict(single_call_items(ta, tok_json, lines, n_visible, want))


_SINGLE_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
import torch
import bench
import tokenizers_amd as ta
tok_json, n_types, _ = bench.load_config(%(config)r)
lines = bench.make_corpus(%(config)r, %(n)d, 100, %(type_seed)d, n_types)
for k, v in bench.single_call_items(ta, tok_json, lines, torch.cuda.device_count(), %(want)d):
    print(json.dumps({k: v}), flush=True)
"""


def single_call_child(config: str, n_lines: int, type_seed: int, want: int, timeout_s: int = 300) -> dict:
    import subprocess
    code = _SINGLE_CHILD % {"root": ROOT, "config": config, "n": n_lines, "type_seed": type_seed, "want": want}
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out, note = "", None
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout_s)
        out = r.stdout
        if r.returncode != 0:
            note = f"child exited with {r.returncode}: {r.stderr[-300:]}"
    except subprocess.TimeoutExpired as ex:
        out = ex.stdout.decode() if isinstance(ex.stdout, bytes) else (ex.stdout or "")
        note = f"child killed after {timeout_s} s (what it had measured by then is kept)"
    res = {}
    for line in out.splitlines():
        line = line.strip()
        if line.startswith("{"):
            try:
                res.update(json.loads(line))
            except Exception:
                pass
    if note:
        res["note"] = note
    return res


# profile stage (capi.cpp Prof) -> the kernel that dominates it, as rocprofv3 names it (prefix match)
KERNEL_OF_STAGE = {"bpe_merge_lds": "k_bpe_merge_lds<16,", "bpe_merge_lds32": "k_bpe_merge_lds<32,", "bpe_merge_lane": "k_bpe_merge_lane<16>",
                   "bpe_merge_lane32": "k_bpe_merge_lane<32>", "bpe_merge16": "k_bpe_merge<16>", "bpe_merge64": "k_bpe_merge<64>",
                   "pretok_gpt2": "k_pretok_gpt2", "pretok_gpt2_seq": "k_pretok_gpt2_seq", "pretok_llama3": "k_pretok_llama3_lane",
                   "pretok_local": "k_pretok_local", "compact": "k_compact", "emit_pretok": "k_emit_pretok", "lookup": "k_lookup",
                   "wordpiece_word_lookup": "k_lookup", "wordlevel_lookup": "k_lookup", "bert_normalize": "k_bn_write",
                   "wordpiece": "k_wordpiece", "added_token_match": "k_added_candidates",
                   "claims_publish": "k_claims_publish", "leadmask_scan": "k_leadmask", "token_meta": "k_token_meta"}


def csrc_sha16() -> str:
    """sha256 over the kernel / host sources the library is built from (tokenizers_amd/csrc, sorted paths): what a committed PMC summary
    is stamped with (tools/pmc_summary.py) -- its traffic figures describe THIS build iff the hashes agree."""
    import hashlib
    h = hashlib.sha256()
    base = os.path.join(ROOT, "tokenizers_amd", "csrc")
    for d, _, files in sorted(os.walk(base)):
        for f in sorted(files):
            if f.endswith((".hip", ".hpp", ".cpp", ".c", ".h", ".inc")):
                h.update(os.path.relpath(os.path.join(d, f), base).encode())
                with open(os.path.join(d, f), "rb") as fh:
                    h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(stage: str, config: str = "c2", suffix: str = ""):
    """HBM-side bytes per launch of the dominant kernel from the newest committed rocprofv3 PMC summary of this config
    (profiles/rN_<config>_pmc_summary.json, written by tools/round_profile.sh): (2*FETCH_SIZE + WRITE_SIZE) KB, the gfx950 correction of
    MI355X_MICROARCH.md -- and where the figure comes from (file, kernel, commit).  (None, None) if no PMC run covers the kernel."""
    import glob
    try:
        paths = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9]_{config}{suffix}_pmc_summary.json")))
        if not paths and not suffix:
            paths = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*{config}*_pmc_summary.json"))) or \
                (sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json"))) if config == "c2" else [])
        if not paths:
            return None, None
        with open(paths[-1]) as fh:
            summary = json.load(fh)
        ks = summary["kernels"]
        want = KERNEL_OF_STAGE.get(stage, "k_" + stage)
        name, k = (want, ks[want]) if want in ks else next(((n, v) for n, v in ks.items() if n.startswith(want)), (None, None))
        if not k:
            return None, None
        # stale = the summary was taken on other kernel sources than the ones this run was built from (hash of tokenizers_amd/csrc; a summary
        # without the hash -- rounds 1-5 -- falls back to comparing its commit with .build_commit)
        if summary.get("csrc_sha16"):
            stale = summary["csrc_sha16"] != csrc_sha16()
        else:
            try:
                with open(os.path.join(ROOT, ".build_commit")) as fh:
                    stale = fh.read().strip().split("+")[0] != str(summary.get("commit")).split("+")[0]
            except OSError:
                stale = True
        src = {"file": os.path.relpath(paths[-1], ROOT), "kernel": name, "commit": summary.get("commit"), "traffic_stale": bool(stale),
               "how": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; (2 * FETCH_SIZE + WRITE_SIZE) per launch (gfx950 correction)"}
        return int(k["hbm_bytes_per_launch"]), src
    except Exception:
        return None, None


_CPU_CHILD = r"""
import json, os, sys, time
sys.path.insert(0, %(root)r)
import tokenizers as ref
from oracle import synth
import bench
tok_json, n_types, _ = bench.load_config(%(config)r)
lines = bench.make_corpus(%(config)r, %(n)d, 100, 0, n_types)[:%(n)d]
rt = ref.Tokenizer.from_str(tok_json)
nbytes = sum(len(s.encode("utf-8")) for s in lines)
rt.encode_batch_fast(lines[:2000], add_special_tokens=False)
t0 = time.perf_counter(); enc = rt.encode_batch_fast(lines, add_special_tokens=False); dt = time.perf_counter() - t0
print(json.dumps({"gbps": nbytes / dt / 1e9, "mtok": sum(len(e.ids) for e in enc) / dt / 1e6, "n": len(lines), "mb": nbytes / 1e6}))
"""


def cpu_baseline(tok_json: str, lines: list[str], cpu_lines: int, config: str = None, brief: bool = False) -> dict:
    """The reference's own encode_batch (Rayon) on a bounded sample of the same corpus: all cores (the headline baseline) plus
    the shapes SURVEY 8d / BASELINE.md section 3 ask for.  ~30 s of CPU work in total."""
    cores = os.cpu_count() or 1
    try:
        import tokenizers as ref
    except Exception:
        ref = None
    if ref is None:
        from oracle import oracle as orc       # C restatement, single thread
        n = cpu_lines or 50_000
        sample = lines[:n]
        o = orc.Oracle(tok_json)
        t0 = time.perf_counter()
        o.encode_batch(sample)
        dt = time.perf_counter() - t0
        nbytes = sum(len(s.encode("utf-8")) for s in sample)
        return {"value": round(nbytes / dt / 1e9, 5), "unit": "GB/s", "cores": 1, "kind": "port",
                "sample": f"oracle/ C restatement, 1 thread, first {n} lines ({nbytes / 1e6:.1f} MB)"}
    rt = ref.Tokenizer.from_str(tok_json)
    n = cpu_lines or len(lines)                        # the identical corpus: ~3 s a pass on the box's 256 cores
    sample = lines[:n]
    nbytes = sum(len(s.encode("utf-8")) for s in sample)
    rt.encode_batch_fast(sample[:20000], add_special_tokens=False)          # warm-up (Rayon pool, caches)

    def best_of(fn, reps, budget_s):
        best, t_all, r = float("inf"), time.time(), None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            best = min(best, time.perf_counter() - t0)
            if time.time() - t_all > budget_s:
                break
        return best, r
    best, enc = best_of(lambda: rt.encode_batch_fast(sample, add_special_tokens=False), 3, 12)
    ntok = sum(len(e.ids) for e in enc)
    del enc
    others = {}
    try:
        b2, _ = best_of(lambda: rt.encode_batch(sample[:200_000], add_special_tokens=False), 2, 8)
        nb2 = sum(len(s.encode("utf-8")) for s in sample[:200_000])
        others["encode_batch_with_offsets_all_cores_gbps"] = round(nb2 / b2 / 1e9, 4)
        if brief:
            raise StopIteration
        # the reference's own criterion shape: 1,000 documents per encode_batch call (benches/bpe_benchmark.rs:17,43; common/mod.rs:35-57)
        sub = sample[:100_000]
        nb3 = sum(len(s.encode("utf-8")) for s in sub)
        t0 = time.perf_counter()
        for k in range(0, len(sub), 1000):
            rt.encode_batch_fast(sub[k:k + 1000], add_special_tokens=False)
        others["encode_batch_fast_1000_docs_per_call_gbps"] = round(nb3 / (time.perf_counter() - t0) / 1e9, 4)
        # one thread: the Rayon pool is process-global, so a fresh process with TOKENIZERS_PARALLELISM=false
        # (bindings/python/benches/test_tiktoken.py:108-116)
        cfg = config or _config_of(tok_json)
        env = dict(os.environ, TOKENIZERS_PARALLELISM="false", RAYON_NUM_THREADS="1")
        r = subprocess.run([sys.executable, "-c", _CPU_CHILD % {"root": ROOT, "config": cfg, "n": 20000}], env=env, capture_output=True, text=True, timeout=120)
        one = json.loads(r.stdout.strip().splitlines()[-1])
        others["encode_batch_fast_1_thread_gbps"] = round(one["gbps"], 5)
        others["encode_batch_fast_1_thread_sample"] = f"{one['n']} lines ({one['mb']:.1f} MB), fresh process, TOKENIZERS_PARALLELISM=false"
    except StopIteration:
        pass
    except Exception as ex:
        others["error"] = repr(ex)
    return {"value": round(nbytes / best / 1e9, 4), "unit": "GB/s", "cores": cores, "kind": "reference",
            "mtokens_per_s": round(ntok / best / 1e6, 3),
            "sample": f"tokenizers=={ref.__version__} Tokenizer.encode_batch_fast(add_special_tokens=False), Rayon on all "
                      f"{cores} host cores, first {n} lines ({nbytes / 1e6:.1f} MB) of the same corpus, best of <=3; "
                      "includes the wheel's Python str->String marshalling and Encoding construction",
            "others": others}


def _config_of(tok_json: str) -> str:
    d = json.loads(tok_json)
    if d["model"].get("type") == "WordPiece":
        return "c3"
    return "c4" if d["model"].get("ignore_merges") else "c2"


if __name__ == "__main__":
    main()
