"""The compaction's prefix sums on the device (run with -m gpu): every document's ids and token CSR against the oracle, at every setting
of the compaction's test hooks.

k_compact (kernels/output.hip, results.hip) places a chunk at its workgroup's own running prefix plus the published totals of the
chunks since the workgroup's previous one -- through one word per group of 64 chunks where the group is complete, through the chunks'
own words where it is not, computing a total itself when its owner does not publish it in time.  One batch through the DEVICE entry
(one pipeline run, one compaction: the host entry would cut it into slices) of 2,600 chunks of 1,024 pre-tokens: two whole rounds of
the resident grid of an MI355X (1,280 workgroups) and forty chunks more, so a workgroup's range of predecessors is a grid wide at the
default setting, one chunk wide at grid 1, a few chunks at 5, a group give or take one at 64 / 65, and everything in front of the
chunk at 100,000 (a workgroup per chunk).  (The handle does not report its grid, hence a fixed chunk count; some 17 MB of text.)
The text: oracle/synth.gen_lines lines with the C2 tokenizer, an unknown 30-letter word spliced into every 97th line (a pre-token of
more than four tokens: its ids travel through tmp_ids), every 50th document empty.

The oracle runs ONCE (module fixture); every hook setting is one child process under a timeout, started like those of
tests/test_liveness_gpu.py: a compaction that waited for ever shows as a failed test, not as a hung session."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, N_CHUNKS = 1024, 2600


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from oracle import synth, oracle as orc
    js = synth.load_or_train_gpt2()
    rng = np.random.default_rng(4711)
    docs = synth.gen_lines(165_000, text_seed=91)
    for i in range(0, len(docs), 97):
        docs[i] += " " + "".join(chr(97 + int(c)) for c in rng.integers(0, 26, 30))
    for i in range(0, len(docs), 50):
        docs[i] = ""
    exp = orc.Oracle(js).encode_batch(docs)
    # pre-tokens per document: the word index of its last token + 1 (every pre-token of a byte-level BPE has a token)
    toff = np.asarray(exp.tok_offsets, dtype=np.int64)
    words = np.asarray(exp.words, dtype=np.int64)
    per_doc = np.where(toff[1:] > toff[:-1], words[np.maximum(toff[1:] - 1, 0)] + 1, 0)
    cum = np.cumsum(per_doc)
    n = int(np.searchsorted(cum, (N_CHUNKS - 1) * CHUNK + CHUNK // 2)) + 1      # the batch ends in the middle of chunk 2,600
    assert n < len(docs) and (N_CHUNKS - 1) * CHUNK < cum[n - 1] <= N_CHUNKS * CHUNK, (n, len(docs))
    n_small = n // 3
    d = tmp_path_factory.mktemp("compact_prefix")
    with open(d / "docs.json", "w", encoding="utf-8") as fh:
        json.dump(docs[:n], fh)
    np.savez(d / "exp.npz", ids=np.asarray(exp.ids[:toff[n]], dtype=np.uint32), tok_offsets=toff[:n + 1], n_pretok=np.int64(cum[n - 1]), n_small=np.int64(n_small))
    return str(d)


_CODE = (
    "import json, numpy as np, torch, tokenizers_amd as ta\n"
    "from oracle import synth\n"
    "d = %r\n"
    "docs = json.load(open(d + '/docs.json', encoding='utf-8'))\n"
    "exp = np.load(d + '/exp.npz')\n"
    "tok = ta.Tokenizer.from_str(synth.load_or_train_gpt2(), device=0)\n"
    "def run(n, check_chunks):\n"
    "    buf, off = ta.pack_documents(docs[:n])\n"
    "    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()\n"
    "    b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), n, int(off[-1]), stream=torch.cuda.current_stream().cuda_stream).sync()\n"
    "    toff = b.tok_offsets_tensor().cpu().numpy()[:n + 1]\n"
    "    ids = b.ids_tensor().cpu().numpy().view('uint32')\n"
    "    t = int(exp['tok_offsets'][n])\n"
    "    if check_chunks: assert (b.n_pretokens + 1023) // 1024 == %d, b.n_pretokens\n"
    "    assert b.n_tokens == t, (b.n_tokens, t)\n"
    "    assert np.array_equal(toff, exp['tok_offsets'][:n + 1]), 'token CSR differs from the oracle'\n"
    "    assert len(ids) == t and np.array_equal(ids, exp['ids'][:t]), 'token ids differ from the oracle'\n"
    "%s"
    "print('PREFIX_OK')\n")

_ONCE = "run(len(docs), True)\n"
# stale group words must not leak: the larger batch leaves every group word it used complete, the smaller one starts from nothing again
_TWICE = "run(len(docs), True)\nrun(int(exp['n_small']), False)\nrun(len(docs), True)\n"
_PHASES = "run(len(docs), True)\nph = tok.debug_phases()['compact']\nassert ph[7] > 0 and ph[2] > 0, ph\n"


def _child(corpus, env, body=_ONCE):
    code = "import sys; sys.path.insert(0, %r)\n" % ROOT + _CODE % (corpus, N_CHUNKS, body)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert "PREFIX_OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def _hooks(**kw):
    return {"TKAMD_TEST_HOOKS": "1", **kw}


@pytest.mark.parametrize("env", [
    {},
    _hooks(TKAMD_CP_GRID="1"), _hooks(TKAMD_CP_GRID="5"), _hooks(TKAMD_CP_GRID="64"), _hooks(TKAMD_CP_GRID="65"), _hooks(TKAMD_CP_GRID="100000"),
    _hooks(TKAMD_LB_PATIENCE="0", TKAMD_CP_GRID="5"), _hooks(TKAMD_LB_PATIENCE="0"),
], ids=["default", "grid-1", "grid-5", "grid-64", "grid-65", "grid-100000", "no-patience-grid-5", "no-patience"])
def test_every_document_equals_the_oracle(corpus, env):
    _child(corpus, env)


def test_phase_timers_instantiation(corpus):
    """the diagnostic instantiation (TKAMD_PHASES): the same result, and its stamps are there"""
    _child(corpus, _hooks(TKAMD_PHASES="1"), _PHASES)


def test_a_smaller_batch_after_a_larger_one_on_one_handle(corpus):
    _child(corpus, {}, _TWICE)
