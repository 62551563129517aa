"""Randomised differential of the whole device path against the reference wheel, without a GPU: the SIMT build of the library
(tests/harness/simt_build.py builds it) encodes random -- deliberately nasty -- Unicode through every fixture family, as single
sequences, pairs, pre-tokenized words and pairs of those, with random truncation / padding sections, and every field of every
encoding (and of its overflowing ones) is compared with what the wheel returns for the same input.  The cases are those of
tests/fuzz_cases.py (make_case(family, n): the n-th draw of this run's seed names the case), whose seeds 0..11 of every family are
recorded in tests/golden/fuzz_layouts_vectors.json.gz and run by the suite.  Test infrastructure: run it for as long as you like; a seed
that fails becomes a test (fuzz_cases.found_cases).

    python tools/fuzz_live.py <seed> <seconds> [fixture,fixture,...]          (default: fuzz_cases.FAMILIES)
"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenizers_amd import _lib  # noqa: E402

if os.environ.get("TKAMD_FUZZ_GPU") != "1":             # (TKAMD_FUZZ_GPU=1 on a GPU box: the product library on cuda:0 instead of the emulation)
    _lib.LIB_PATH = os.path.join(ROOT, "tests", "harness", "_libtokenizers_amd_simt.so")
import tokenizers as ref  # noqa: E402

import tokenizers_amd as ta  # noqa: E402
from tests import fuzz_cases as fc  # noqa: E402

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
budget = float(sys.argv[2]) if len(sys.argv) > 2 else 120
names = sys.argv[3].split(",") if len(sys.argv) > 3 else list(fc.FAMILIES)
rnd = random.Random(seed)
heavy = os.environ.get("FUZZ_TRUNCATION") == "1"       # (mostly truncated batches, short windows, wider strides)


def fields(e):
    return (e.ids, e.type_ids, e.attention_mask, e.special_tokens_mask, [tuple(o) for o in e.offsets], e.word_ids, e.sequence_ids)


def deep(e):
    return [fields(e)] + [fields(o) for o in e.overflowing]


t0 = time.time()
n_cases = n_docs = n_ref = n_refused = n_dec = 0
while time.time() - t0 < budget:
    name = rnd.choice(names)
    case = fc.make_case(name, f"live:{seed}:{rnd.getrandbits(48)}", heavy_truncation=heavy)
    js, inputs, special, pre = case["json"], fc.call_inputs(case), case["add_special_tokens"], case["is_pretokenized"]
    d = json.loads(js)
    try:
        tok = ta.Tokenizer.from_str(js, device=0)
    except ta.UnsupportedError:
        continue
    rt = ref.Tokenizer.from_str(js)
    rt.encode_special_tokens = tok.encode_special_tokens = case["encode_special_tokens"]
    ctx = (name, case["seed"], rt.encode_special_tokens, d.get("truncation"), d.get("padding"), case["mode"], special, d.get("post_processor"), d.get("normalizer"), d.get("pre_tokenizer"), {k: v for k, v in d["model"].items() if k not in ("vocab", "merges")}, d["added_tokens"][-4:])
    try:
        exp = rt.encode_batch(inputs, add_special_tokens=special, is_pretokenized=pre)
    except BaseException as e:          # (a TruncationError, or the stride assert's panic)
        try:
            tok.encode_batch(inputs, add_special_tokens=special, is_pretokenized=pre)
            print("REF RAISED, WE DID NOT", ctx, repr(e)[:200], inputs)
            sys.exit(1)
        except (ValueError, ta.TokenizersAmdError):
            n_ref += 1
            continue
    try:
        got = tok.encode_batch(inputs, add_special_tokens=special, is_pretokenized=pre)
    except ta.UnsupportedError as e:
        n_refused += 1
        print("REFUSED", ctx, str(e)[:160])
        continue
    except Exception as e:
        print("WE RAISED", ctx, repr(e)[:300], inputs)
        sys.exit(1)
    for i, e in enumerate(exp):
        if deep(e) != deep(got[i]):
            print("MISMATCH", ctx, repr(inputs[i]))
            json.dump({"name": name, "seed": case["seed"], "json": js, "inputs": case["inputs"], "index": i, "special": special, "pre": pre, "esp": rt.encode_special_tokens}, open(f"/tmp/fuzz_fail_{seed}.json", "w"), ensure_ascii=False)
            a, b = deep(e), deep(got[i])
            print(" encodings", len(a), len(b))
            for k, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    for fname, fx, fy in zip(("ids", "type", "att", "spm", "offs", "words", "seq"), x, y):
                        if fx != fy:
                            print("  enc", k, fname, "\n   ref", fx, "\n   got", fy)
                    break
            sys.exit(1)
    # decode_batch of what was encoded (and of the ids shuffled: sequences no encoder would produce)
    seqs = [e.ids for e in exp] + [rnd.sample(e.ids, len(e.ids)) for e in exp[:4]]
    skip = rnd.random() < 0.5
    try:
        dexp = rt.decode_batch(seqs, skip_special_tokens=skip)
    except BaseException as e:
        dexp = None
    try:
        dgot = tok.decode_batch(seqs, skip_special_tokens=skip)
        n_dec += 1
    except ta.UnsupportedError:
        dgot = dexp
    if dexp is not None and dexp != dgot:
        for x, y, q in zip(dexp, dgot, seqs):
            if x != y:
                print("DECODE MISMATCH", name, skip, q, "\n ref", repr(x), "\n got", repr(y))
                sys.exit(1)
    n_cases += 1
    n_docs += len(inputs)
print("ok seed", seed, "cases", n_cases, "inputs", n_docs, "reference errors matched", n_ref, "refused", n_refused, "decoded", n_dec, flush=True)
