"""Writes tests/golden/fuzz_layouts_vectors.json.gz: what the reference wheel answers to the cases of tests/fuzz_cases.py -- seeds 0..11 of
every family, and the reduced cases of what the differential found -- and, for the cases this library refuses, the first characters of
its message (so a case that newly loads, or newly refuses, fails tests/test_fuzz_layouts_gpu.py instead of skipping).  The tokenizer files
are not stored again: a case is a name and a seed, pinned by the SHA-256 of what the generator makes of them.

    python tools/make_golden_fuzz.py          (needs the wheel; the library's refusals are asked of the SIMT build, tests/harness/simt_build.py,
                                               or with TKAMD_FUZZ_GPU=1 of the product library on device 0)
"""
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenizers_amd import _lib  # noqa: E402

if os.environ.get("TKAMD_FUZZ_GPU") != "1":
    _lib.LIB_PATH = os.path.join(ROOT, "tests", "harness", "_libtokenizers_amd_simt.so")
import tokenizers as ref  # noqa: E402

import tokenizers_amd as ta  # noqa: E402
from tests import fuzz_cases as fc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fuzz_layouts_vectors.json.gz")


def record(case):
    """the wheel's answers to one case, and whether the library takes it"""
    rec = {"digest": fc.digest(case), "refused": None, "raised": False, "enc": None, "dec": None}
    kw = dict(add_special_tokens=case["add_special_tokens"], is_pretokenized=case["is_pretokenized"])
    try:
        tok = ta.Tokenizer.from_str(case["json"], device=0)
        tok.encode_special_tokens = case["encode_special_tokens"]
        try:
            tok.encode_batch(fc.call_inputs(case), **kw)
        except ta.UnsupportedError as e:         # (refused at the call: a single template the path does not take, ...)
            rec["refused"] = ("encode: " + str(e))[:fc.REFUSAL_CHARS]
        except (ValueError, ta.TokenizersAmdError):
            pass
    except ta.UnsupportedError as e:
        rec["refused"] = str(e)[:fc.REFUSAL_CHARS]
    rt = ref.Tokenizer.from_str(case["json"])
    rt.encode_special_tokens = case["encode_special_tokens"]
    try:
        exp = rt.encode_batch(fc.call_inputs(case), **kw)
    except BaseException:             # (a TruncationError, or the stride assert's panic)
        rec["raised"] = True
        return rec
    rec["enc"] = [fc.deep(e) for e in exp]
    seqs = fc.decode_sequences(case, [e.ids for e in exp])
    rec["dec"] = []
    for skip in (False, True):
        try:
            rec["dec"].append(rt.decode_batch(seqs, skip_special_tokens=skip))
        except BaseException:
            rec["dec"].append(None)
    return rec


def main():
    out = {"seeds": list(fc.SEEDS), "families": {}, "found": {}}
    t0 = time.time()
    short = []
    for name in fc.FAMILIES:
        t1 = time.time()
        recs = [record(fc.make_case(name, seed)) for seed in fc.SEEDS]
        out["families"][name] = recs
        n_ref = sum(1 for r in recs if r["refused"] is not None)
        print(f"{name:34s} compared {len(recs) - n_ref:2d} refused {n_ref:2d} wheel raised {sum(r['raised'] for r in recs):2d}  {time.time() - t1:5.1f} s", flush=True)
        short += [name] if len(recs) - n_ref < 8 else []
    for finding, cases in fc.found_cases().items():
        out["found"][finding] = [record(c) for c in cases]
    blob = json.dumps(out, ensure_ascii=False, separators=(",", ":")).encode("utf-8")
    with open(OUT, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", compresslevel=9, mtime=0, filename="") as gz:
            gz.write(blob)
    assert not short, f"fewer than 8 of 12 cases load for {short}: lower the mixing probabilities of what these families refuse (tests/fuzz_cases.py)"
    print(f"{OUT}: {os.path.getsize(OUT)} bytes ({len(blob)} of JSON), {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
