"""-m gpu: k_pretok_gpt2_seq, one lane per 64-byte mask word (kernels/pretok_gpt2.hip), through the device entry with the GPT-2
test tokenizer.  Ids + byte offsets + word ids expose every pre-token boundary; every document is compared with the CPU oracle.
The shapes are the ones at which the kernel takes another path: a lane ends every 64 bytes (halo by shuffle), a wavefront every
4,096 (halo through LDS), a workgroup every 16,384 (threads 0 and 1 classify the bytes beyond it), and the text ends anywhere."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import synth
from tests import gpt2_word_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpt2():
    import tokenizers_amd as ta
    js = synth.load_or_train_gpt2()
    return ta.Tokenizer.from_str(js, device=0), orc.Oracle(js)


def _check(gpt2, docs, char=False):
    import torch
    import tokenizers_amd as ta
    tok, oracle = gpt2
    buf, off = ta.pack_documents(docs)
    d_text, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    b = tok.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), int(off[-1]), stream=torch.cuda.current_stream().cuda_stream,
                                offsets="char" if char else "byte", word_ids=True).sync()
    exp = oracle.encode_batch(docs, char_offsets=char)
    to = b.tok_offsets_tensor().cpu().numpy()
    eo = np.asarray(exp.tok_offsets)
    n_tok = int(eo[-1])
    ids = b.ids_tensor().cpu().numpy().view(np.uint32)[:n_tok]
    offs = b.offsets_tensor().cpu().numpy().view(np.uint32).reshape(-1, 2)[:n_tok]
    wid = b.word_ids_tensor().cpu().numpy().view(np.uint32)[:n_tok]
    if not np.array_equal(to, eo):
        d = int(np.nonzero(np.diff(to) != np.diff(eo))[0][0])
        raise AssertionError(f"document {d} of {len(docs)} (bytes {off[d]}..{off[d + 1]}): {to[d + 1] - to[d]} tokens, the oracle has {eo[d + 1] - eo[d]}: {docs[d][:80]!r}")
    for what, got, want in (("ids", ids, np.asarray(exp.ids)), ("offsets", offs, np.asarray(exp.offsets).reshape(-1, 2)), ("word ids", wid, np.asarray(exp.words))):
        neq = got != want                                    # (no token at all: empty arrays, nothing to reshape)
        bad = np.nonzero(neq.any(axis=1) if neq.ndim > 1 else neq)[0]
        if len(bad):
            d = int(np.searchsorted(eo, bad[0], side="right") - 1)
            raise AssertionError(f"{what} of document {d} of {len(docs)} (bytes {off[d]}..{off[d + 1]}): {docs[d][:80]!r}")


def _docs_of_length(n, seed):
    """documents over the adversarial alphabet, n bytes in all"""
    docs, total = [], 0
    for d in gc.random_docs(4000, seed, max_len=60):
        b = len(d.encode("utf-8"))
        if total + b > n:
            break
        docs.append(d)
        total += b
    docs.append("it's x" * ((n - total) // 6) + "y" * ((n - total) % 6))
    return docs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 17])
def test_total_text_length(gpt2, n):
    docs = _docs_of_length(n, 800 + n % 11)
    assert sum(len(d.encode("utf-8")) for d in docs) == n
    _check(gpt2, docs)


@pytest.mark.parametrize("kind", ["lane", "wave", "group"])
def test_document_boundary_around_every_edge(gpt2, kind):
    """a document ends at every offset from -8 to +8 around an edge of the kind (and many more elsewhere)"""
    edges = gc.edges_of(kind)[:17]
    docs, total = [], 0
    pool = iter(gc.random_docs(40000, 810, max_len=50))
    for e, delta in zip(edges, range(-8, 9)):
        target = e + delta
        while True:
            d = next(pool)
            b = len(d.encode("utf-8"))
            if total + b > target:
                break
            docs.append(d)
            total += b
        docs.append(("we'll go " * 40)[:target - total])       # (a document of the pool is 200 bytes at the most)
        total = target
    docs.append(" and the rest of it's here")
    assert all(e + k in set(np.cumsum([len(d.encode("utf-8")) for d in docs]).tolist()) for e, k in zip(edges, range(-8, 9)))
    _check(gpt2, docs)


@pytest.mark.parametrize("kind", ["lane", "wave", "group"])
def test_straddling_cases(gpt2, kind):
    """the constructed cases of tests/test_pretok_gpt2_words.py: a multi-byte code point, a contraction, spaces in front of a letter and a
    document start at every offset from -8 to +8 around an edge of the kind"""
    text, off = gc.straddling_text(gc.edges_of(kind))
    _check(gpt2, gc.docs_of(text, off))


def test_straddling_cases_with_char_offsets(gpt2):
    """the instantiation that writes the lead-byte mask too (char offsets count in it)"""
    text, off = gc.straddling_text(gc.edges_of("lane"))
    _check(gpt2, gc.docs_of(text, off), char=True)
    _check(gpt2, _docs_of_length(16385, 820) + _docs_of_length(4097, 821), char=True)


def test_empty_documents(gpt2):
    body = _docs_of_length(5000, 830)
    _check(gpt2, [""] + body)
    _check(gpt2, body + [""])
    _check(gpt2, body[:7] + [""] + body[7:])
    _check(gpt2, ["", ""] + body[:3] + ["", ""] + body[3:] + ["", ""])
    _check(gpt2, [""])
    _check(gpt2, ["", "", ""])
