#!/usr/bin/env python3
"""Records tests/golden/hot_table_eligible.json: per tokenizer, which token ids are ELIGIBLE for the hot-word table (settled words of
<= 12 bytes -- for byte-level BPE that needs the load-time proof of the whole-word table, which runs the device merge kernel), the tables'
hash seed, and the load-time table itself as a SHA-256 and its word count.  tests/test_hot_table_core.py rebuilds the table from these on
the CPU.  A RECORDED RESULT of the library that is loaded: on an MI355X the product, with --simt the host build of the same csrc/ under
the emulation of the tests (no GPU needed; the 128 k vocabulary takes a few minutes to load there).

  python tools/make_golden_hot_table.py [--simt]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["gpt2_synth_50257", "bert_wordpiece_30522", "llama3_128k"]
OUT = os.path.join(ROOT, "tests", "golden", "hot_table_eligible.json")


def main():
    os.environ["TKAMD_HOT_ADAPT"] = "0"
    if "--simt" in sys.argv:
        from tests.harness import simt_build
        from tokenizers_amd import _lib
        _lib.LIB_PATH, _lib._lib = simt_build.build(), None
    import tokenizers_amd as ta
    from tests.helpers import load_tokenizer_json
    out = {"_about": "RECORDED RESULT (tools/make_golden_hot_table.py): eligible = a bit per token id, little endian inside a byte, hex"}
    for name in NAMES:
        tok = ta.Tokenizer.from_str(load_tokenizer_json(name), device=0)
        h = tok.hot_table(words=True)
        bits = bytearray((max(h["eligible_ids"]) >> 3) + 1)
        for i in h["eligible_ids"]:
            bits[i >> 3] |= 1 << (i & 7)
        out[name] = {"word_seed": h["word_seed"], "slots": h["slots"], "n_hot": h["n_hot"], "n_eligible": len(h["eligible_ids"]),
                     "blob_sha256": hashlib.sha256(h["blob"]).hexdigest(), "eligible": bytes(bits).hex()}
        print(name, {k: v for k, v in out[name].items() if k != "eligible"}, flush=True)
    with open(OUT, "w", encoding="utf-8") as fh:
        json.dump(out, fh, sort_keys=True, indent=0)
        fh.write("\n")


if __name__ == "__main__":
    main()
