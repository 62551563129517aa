"""Writes tests/golden/host_model_outcomes.json.gz: what HostModel::from_json (tokenizers_amd/csrc/host_model.cpp) makes of every file of
the corpus of tests/host_model_cases.py -- for a file it loads the config and the content digest of tests/harness/host_model_digest.cpp,
for one it refuses the status and the whole message.  The layout digest is not recorded: it depends on the iteration order of
std::unordered_map in the libstdc++ the harness was built against, and serves comparisons of two builds on one machine
(--layout OUT writes "key<TAB>status<TAB>..." lines with all three digests to OUT instead of the golden file; --host-model FILE builds
the harness against another copy of host_model.cpp).

    python tools/make_golden_host_model.py          (g++ alone: no wheel, no GPU)
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import host_model_cases as hc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "host_model_outcomes.json.gz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", metavar="OUT")
    ap.add_argument("--host-model", metavar="FILE")
    args = ap.parse_args()
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        exe = hc.build_harness(os.path.join(tmp, "host_model_digest"), host_model_cpp=args.host_model)
        items = [kv for group in hc.GROUPS.values() for kv in group()]
        got = hc.run_harness(exe, items, tmp, layout=bool(args.layout))
    assert len(got) == len(items), "two files of the corpus share a key"
    n_ok = sum(1 for r in got.values() if r["status"] == "OK")
    if args.layout:
        with open(args.layout, "w", encoding="utf-8") as fh:
            for key in sorted(got):
                fh.write(key + "\t" + "\t".join(got[key].values()) + "\n")
        print(f"{args.layout}: {len(got)} lines ({n_ok} load), {time.time() - t0:.0f} s")
        return
    blob = json.dumps(got, ensure_ascii=False, sort_keys=True, separators=(",", ":")).encode("utf-8")
    with open(OUT, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", compresslevel=9, mtime=0, filename="") as gz:
            gz.write(blob)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes ({len(blob)} of JSON), {len(got)} files ({n_ok} load), {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
