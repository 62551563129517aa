"""Records the reference wheel's answers for the cases of tests/dense_cases.py in tests/golden/dense_vectors.json.gz: per case the
Encodings of encode_batch stacked into [n_rows, width] lists -- ids, attention_mask, type_ids, special_tokens_mask, offsets, word_ids
(None -> -1) -- under the transformers key names, or, for the cases of DIGEST_ONLY, their digest.  Runs on the CPU with the wheel:
    python tools/make_golden_dense.py"""
import gzip
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import dense_cases as dn
from tests.helpers import GOLD


def stacked(case) -> dict:
    import tokenizers
    tk = tokenizers.Tokenizer.from_str(dn.tokenizer_json(case))
    encs = tk.encode_batch(list(case["inputs"]), add_special_tokens=case["add_special_tokens"])
    out = {"input_ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs], "token_type_ids": [e.type_ids for e in encs],
           "special_tokens_mask": [e.special_tokens_mask for e in encs], "offset_mapping": [[list(o) for o in e.offsets] for e in encs],
           "word_ids": [[-1 if w is None else w for w in e.word_ids] for e in encs]}
    for e in encs:
        assert len(e.ids) == case["width"], (case["name"], len(e.ids), case["width"])
    return out


def digest(rows: dict) -> str:
    """sha256 over the six arrays as little-endian int64, in the order of dense_cases.FIELDS"""
    import numpy as np
    h = hashlib.sha256()
    for k in dn.FIELDS:
        h.update(np.asarray(rows[k], dtype="<i8").tobytes())
    return h.hexdigest()


if __name__ == "__main__":
    import tokenizers
    cases = {}
    for c in dn.CASES:
        rows = stacked(c)
        cases[c["name"]] = {"digest": digest(rows), "n_rows": len(c["inputs"])} if c["name"] in dn.DIGEST_ONLY else rows
    out = {"_about": "the reference wheel's encode_batch for tests/dense_cases.py, stacked per field (tools/make_golden_dense.py)",
           "tokenizers_version": tokenizers.__version__, "cases": cases}
    path = os.path.join(GOLD, "dense_vectors.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps(out, separators=(",", ":")).encode("utf-8"))
    print(path, os.path.getsize(path), "bytes;", len(cases), "cases")
